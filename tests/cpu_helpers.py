"""What the CPU test modules of the libraries share: where the LLVM tools are, the C compiler, the check that a library is built,
the defined dynamic symbols of a library, and the walker that reads the case ids a GPU test module runs from its syntax tree."""
import ast
import os
import subprocess

LLVM = "/opt/rocm/lib/llvm/bin"


def need_lib(path):
    # (the library is a build product: __graft_entry__.build() makes it; a tree that was never built has nothing to inspect)
    assert os.path.exists(path), "%s is not built (python -m ubresnet_amd.build)" % os.path.basename(path)


def cc(plus=False):
    c = os.path.join(LLVM, "clang++" if plus else "clang")
    return c if os.path.exists(c) else ("c++" if plus else "cc")


def readelf(*args):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf")] + list(args), capture_output=True, text=True, check=True).stdout


def defined_symbols(path):
    """the names of the dynamic symbols that the library defines"""
    rows = [l.split() for l in readelf("--dyn-syms", "-W", path).split("\n")]
    return [r[-1] for r in rows if len(r) == 8 and r[6] != "UND"]


def case_ids_run_by_the_gpu_module(path, table="CASES", call="_run"):
    """the ids that the test functions of the GPU test module at `path` pass to `call`() as first argument, from its syntax tree
    (text in comments or strings does not count): a literal, or a parameter whose values the parametrize decorator lists.
    The module must bind `table` to the case table of its reference module."""
    tree = ast.parse(open(path).read())
    assert any(isinstance(n, ast.Assign) and ast.unparse(n) == "%s = R.KERNEL_CASES" % table for n in tree.body)
    ran = set()
    for node in tree.body:
        if not (isinstance(node, ast.FunctionDef) and node.name.startswith("test_")):
            continue
        params = {}
        for d in node.decorator_list:
            if isinstance(d, ast.Call) and ast.unparse(d.func).endswith("parametrize"):
                try:
                    names, values = ast.literal_eval(d.args[0]), ast.literal_eval(d.args[1])
                except ValueError:         # computed values (the argument-error names): no case ids there
                    continue
                names = [n.strip() for n in names.split(",")] if isinstance(names, str) else list(names)
                for row in values:
                    row = row if len(names) > 1 else (row,)
                    for n, v in zip(names, row):
                        params.setdefault(n, []).append(v)
        for c in ast.walk(node):
            if isinstance(c, ast.Call) and isinstance(c.func, ast.Name) and c.func.id == call:
                a = c.args[0]
                if isinstance(a, ast.Constant):
                    ran.add(a.value)
                else:
                    assert isinstance(a, ast.Name) and a.id in params, "cannot tell the case id of %s" % ast.unparse(c)
                    ran.update(params[a.id])
    return ran
