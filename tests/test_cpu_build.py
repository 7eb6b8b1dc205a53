"""The build table, the shared loader and the entry point without a GPU, for every library of ubresnet_amd.build.LIBS alike: the
table's entries and the partition of csrc/ they make; header lists that are the #include closure of the sources; the compile and
link commands of build(); the built libraries (self-contained, exporting exactly their binding's symbols); a missing library or
a missing symbol is a RuntimeError of the binding; __graft_entry__.build() by what it does."""
import ast
import ctypes as C
import hashlib
import importlib
import importlib.util
import os
import re
import subprocess

import pytest

import cpu_helpers as H
from ubresnet_amd import build as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "ubresnet_amd")
NAMES = list(B.LIBS)
SATELLITES = NAMES[1:]
VERSIONS = dict({n: 1 for n in NAMES}, hip=2)


def _binding(name):
    return importlib.import_module("ubresnet_amd." + B.LIBS[name].binding).BINDING


# ------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------
def test_the_table_names_the_fourteen_libraries_in_build_order():
    assert NAMES == ["hip", "post", "data", "aug", "opt", "weight", "group", "ema", "accum", "stats", "loss", "dice", "tta", "det"]
    hip = B.LIBS["hip"]
    assert hip.out is B.OUT and hip.sources is B.SOURCES and hip.headers is B.HEADERS and hip.binding == "_lib"
    assert B.SOURCES == ["ubr_conv.hip", "ubr_aspp.hip", "ubr_wgrad.hip", "ubr_elem.hip", "ubr_head.hip", "ubr_tape.hip"]
    assert "-ffp-contract=off" in B.FLAGS and "--offload-arch=gfx950" in B.FLAGS
    patterns = open(os.path.join(REPO, ".gitignore")).read().split()
    assert "*.so" in patterns and "*.o" in patterns          # the build products stay out of git


@pytest.mark.parametrize("name", NAMES)
def test_table_entry(name):
    lib = B.LIBS[name]
    assert os.path.basename(lib.out) == "libubresnet_%s.so" % name and os.path.dirname(lib.out) == os.path.dirname(B.OUT) == PKG
    assert os.path.exists(os.path.join(PKG, lib.binding + ".py"))
    assert any(h.endswith(os.path.join("include", "ubresnet_%s.h" % name)) for h in lib.headers)
    if name != "hip":
        assert lib.sources == ["ubr_%s.hip" % name] and lib.binding == "_" + name     # every satellite has exactly one .hip
        assert getattr(B, name.upper() + "_OUT") == lib.out                            # the path's older name still reads the table
        assert not hasattr(B, name.upper() + "_SOURCES") and not hasattr(B, "build_" + name)


def test_the_sources_partition_csrc():
    every = [s for lib in B.LIBS.values() for s in lib.sources]
    assert len(every) == len(set(every)) == 19, "a source belongs to two libraries"
    assert sorted(every) == sorted(f for f in os.listdir(B.CSRC) if f.endswith(".hip")), "a .hip under csrc/ that no library builds"


def _include_closure(files):
    seen, todo = set(), [os.path.realpath(f) for f in files]
    while todo:
        f = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), flags=re.M):
            p = os.path.realpath(os.path.join(os.path.dirname(f), inc))
            if p not in seen:
                seen.add(p)
                todo.append(p)
    return seen


@pytest.mark.parametrize("name", NAMES)
def test_headers_are_what_the_sources_include(name):
    """transitively, through quoted #includes: so a header of one library is in no other library's list unless its sources read it"""
    lib = B.LIBS[name]
    listed = [os.path.realpath(os.path.join(B.CSRC, h)) for h in lib.headers]
    assert len(listed) == len(set(listed))
    assert set(listed) == _include_closure(os.path.join(B.CSRC, s) for s in lib.sources)


def test_source_hash_covers_the_network_only():
    mine = set(B.SOURCES + B.HEADERS)
    for name in SATELLITES:
        assert not mine & set(B.LIBS[name].sources + B.LIBS[name].headers), name
        assert not any(name in os.path.basename(f) for f in mine), name
    # source_hash() reads SOURCES and HEADERS only: a hash over those files by hand is the same
    h = hashlib.sha256()
    for f in sorted(B.SOURCES) + sorted(B.HEADERS):
        with open(os.path.join(B.CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    assert B.source_hash() == h.hexdigest()


# ------------------------------------------------------------------------------------------------------------------------
# the commands
# ------------------------------------------------------------------------------------------------------------------------
def _record(monkeypatch, **kw):
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    built = B.build(force=True, verbose=False, **kw)
    monkeypatch.undo()
    return built, [c for c in lines if "-c" in c], [c for c in lines if "-shared" in c], lines


def _check_commands(lib, compiles, links):
    objs = [os.path.join(B.CSRC, s.replace(".hip", ".o")) for s in lib.sources]
    assert len(compiles) == len(lib.sources) and len(links) == 1
    for cmd, s, obj in zip(compiles, lib.sources, objs):
        assert cmd[0] == B.HIPCC and all(f in cmd for f in B.FLAGS), "compiled with the shared FLAGS"
        assert cmd[-4:] == ["-c", os.path.join(B.CSRC, s), "-o", obj]
    link = links[0]
    assert link[0] == B.HIPCC and "-shared" in link and link[link.index("-o") + 1] == lib.out
    assert [a for a in link if a.endswith(".o")] == objs == link[-len(objs):], "links exactly its own objects"


@pytest.mark.parametrize("name", NAMES)
def test_build_only_compiles_and_links_that_library_and_nothing_else(name, monkeypatch):
    lib = B.LIBS[name]
    built, compiles, links, lines = _record(monkeypatch, only=[name])
    assert built == [lib.out] and len(lines) == len(lib.sources) + 1
    _check_commands(lib, compiles, links)


def test_a_forced_build_of_the_table_is_nineteen_compiles_and_fourteen_links(monkeypatch):
    built, compiles, links, lines = _record(monkeypatch)
    assert built == [lib.out for lib in B.LIBS.values()]
    assert len(compiles) == 19 and len(links) == 14 and len(lines) == 33
    assert [l[l.index("-o") + 1] for l in links] == built, "each output once, in table order"
    at = 0
    for lib, link in zip(B.LIBS.values(), links):
        _check_commands(lib, compiles[at:at + len(lib.sources)], [link])
        at += len(lib.sources)
    with pytest.raises(ValueError, match="no library named"):
        B.build(only=["nope"])


def test_the_command_line_builds_the_table_once_and_prints_the_paths(monkeypatch, capsys):
    import runpy
    lines, real = [], subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, **k: (lines.append(list(cmd)), real(["true"], **k))[1])
    monkeypatch.setattr("sys.argv", ["build.py", "--force"])
    capsys.readouterr()
    runpy.run_module("ubresnet_amd.build", run_name="__main__")
    monkeypatch.undo()
    out = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 33 and sorted(out[:33]) == sorted(" ".join(c) for c in lines)      # (the pool echoes in any order)
    assert out[33:] == [lib.out for lib in B.LIBS.values()]


# ------------------------------------------------------------------------------------------------------------------------
# the built libraries and their bindings
# ------------------------------------------------------------------------------------------------------------------------
def test_no_two_bindings_share_a_prefix_or_a_variable():
    bindings = [_binding(n) for n in NAMES]
    prefixes = [bd.prefix for bd in bindings]
    assert len(set(prefixes)) == 14 and all(re.fullmatch(r"ub[a-z]", p) for p in prefixes)
    assert prefixes == ["ubr", "ubp", "ubd", "uba", "ubo", "ubw", "ubg", "ube", "ubc", "ubs", "ubl", "ubk", "ubt", "ubx"]
    assert [bd.path for bd in bindings] == [lib.out for lib in B.LIBS.values()]


@pytest.mark.parametrize("name", NAMES)
def test_library_stands_alone_and_exports_exactly_its_bindings_symbols(name):
    lib, bd = B.LIBS[name], _binding(name)
    mod = importlib.import_module("ubresnet_amd." + lib.binding)
    assert (mod.LIB_PATH, mod.SYMBOLS, mod.lib, mod.check) == (bd.path, bd.symbols, bd.lib, bd.check)
    assert bd.symbols == list(bd.table) and len(set(bd.symbols)) == len(bd.symbols)
    assert bd.table[bd.prefix + "_last_error"] == (C.c_char_p, []) and bd.table[bd.prefix + "_version"] == (C.c_int, [])
    if name != "hip":
        assert bd.symbols[-2:] == [bd.prefix + "_last_error", bd.prefix + "_version"]
    H.need_lib(lib.out)
    # it links against none of the others
    assert "libubresnet_" not in H.readelf("-d", lib.out).replace("libubresnet_" + name, ""), name
    loaded = bd.lib()
    assert all(hasattr(loaded, s) for s in bd.symbols)
    for s, (restype, argtypes) in bd.table.items():
        assert getattr(loaded, s).restype is restype and getattr(loaded, s).argtypes == argtypes, s
    assert bd.version() == getattr(loaded, bd.prefix + "_version")() == VERSIONS[name]
    # the exports that carry any library's prefix are exactly the declared ones.  The network's library also exports its
    # internal helper ubr_set_error (ubr_host.h shares it between translation units), which the public header does not declare:
    # there the rule is the one tests/test_cpu_host.py has always had, every declared symbol exported, and that one extra named
    prefixed = sorted(n for n in H.defined_symbols(lib.out) if re.match(r"ub[a-z]_", n))
    assert prefixed == sorted(bd.symbols + (["ubr_set_error"] if name == "hip" else []))
    with pytest.raises(RuntimeError, match=r"HIP call failed \(-1\) probe"):
        bd.check(-1, "probe")
    bd.check(0, "probe")


@pytest.mark.parametrize("name", NAMES)
def test_a_missing_library_is_a_runtime_error(name, monkeypatch):
    """a fresh execution of the binding's file with its environment variable pointing nowhere: no fallback"""
    lib, bd = B.LIBS[name], _binding(name)
    nowhere = os.path.join(REPO, "no_such_dir", os.path.basename(lib.out))
    monkeypatch.setenv(bd.prefix.upper() + "_LIB", nowhere)
    spec = importlib.util.spec_from_file_location("ubresnet_amd.%s_missing" % lib.binding, os.path.join(PKG, lib.binding + ".py"))
    fresh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fresh)
    assert fresh.LIB_PATH == nowhere and fresh.BINDING is not bd
    with pytest.raises(RuntimeError, match="is missing; build it with `python -m ubresnet_amd.build`") as e:
        fresh.lib()
    assert nowhere in str(e.value) and "There is no CPU fallback" in str(e.value)
    with pytest.raises(RuntimeError, match="is missing"):
        fresh.check(-1, "probe")


def test_a_file_that_is_no_library_cannot_be_loaded(tmp_path, monkeypatch):
    from ubresnet_amd._binding import Binding
    junk = tmp_path / "libubresnet_junk.so"
    junk.write_bytes(b"not an ELF file")
    monkeypatch.setenv("UBJ_LIB", str(junk))
    with pytest.raises(RuntimeError, match="cannot load %s" % re.escape(str(junk))):
        Binding("UBJ_LIB", "libubresnet_junk.so", "ubj", {}).lib()


@pytest.mark.parametrize("name", NAMES)
def test_a_library_that_lacks_a_declared_symbol_is_a_runtime_error(name):
    from ubresnet_amd._binding import Binding
    lib, bd = B.LIBS[name], _binding(name)
    H.need_lib(lib.out)
    more = Binding("UB__LIB", os.path.basename(lib.out), bd.prefix, dict(bd.table, **{bd.prefix + "_no_such_call": (C.c_int, [])}))
    with pytest.raises(RuntimeError, match="lacks symbols") as e:
        more.lib()
    assert lib.out in str(e.value) and bd.prefix + "_no_such_call" in str(e.value) and bd.symbols[0] not in str(e.value)


@pytest.mark.parametrize("file", ["_binding.py"] + ["_%s.py" % n for n in SATELLITES])
def test_bindings_do_not_import_torch(file):
    tree = ast.parse(open(os.path.join(PKG, file)).read())
    names = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
    names += [n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    roots = [str(n).split(".")[0] for n in names]
    assert "torch" not in roots
    if file == "_binding.py":
        assert sorted(roots) == ["__future__", "ctypes", "os", "threading"]
    else:
        assert "_binding" in names


# ------------------------------------------------------------------------------------------------------------------------
# the entry point
# ------------------------------------------------------------------------------------------------------------------------
def test_entry_point_builds_the_table_once_and_reports_every_library(monkeypatch, capsys):
    import __graft_entry__ as entry
    for lib in B.LIBS.values():
        H.need_lib(lib.out)
    calls = []
    monkeypatch.setattr(B, "build", lambda *a, **kw: calls.append((a, kw)))
    entry.build()
    assert len(calls) == 1 and not calls[0][0] and not calls[0][1].get("only"), "one call, for the whole table"
    lines = capsys.readouterr().out.strip().split("\n")
    assert lines == ["built %s ABI version %d" % (B.LIBS[n].out, VERSIONS[n]) for n in NAMES]


def test_entry_point_refuses_a_library_that_lacks_a_symbol(monkeypatch):
    import __graft_entry__ as entry
    bd = _binding("det")
    H.need_lib(bd.path)
    monkeypatch.setattr(B, "build", lambda *a, **kw: None)
    monkeypatch.setitem(bd.table, "ubx_no_such_call", (C.c_int, []))
    monkeypatch.setattr(bd, "_lib", None)                      # not loaded yet: the next lib() resolves the table again
    with pytest.raises(RuntimeError, match="lacks symbols") as e:
        entry.build()
    assert "libubresnet_det.so" in str(e.value) and "ubx_no_such_call" in str(e.value)
