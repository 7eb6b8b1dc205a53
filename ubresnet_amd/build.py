"""Build the package's shared libraries with hipcc for gfx950, in-tree.

    python -m ubresnet_amd.build [--force] [--addons] [--extras]

LIBS is the table of them, in build order: name -> (out, sources, headers, binding).  `hip` is libubresnet_hip.so, all HIP kernels
of the network and its C ABI; every other entry is a library of one .hip file that links against none of the
others (csrc/ubr_sat.h is the support header they all include; the event-product libraries of csrc/extra/ also share
csrc/ubr_wave.h, their wave and workgroup primitives, and csrc/ubr_scan_plan.h, the plan of their pixel-block compaction; moment,
overlap and match also csrc/ubr_walk_plan.h, ubr_adc_rule.h and ubr_walk.h, their pixel walk and weight rule), and whose purpose the docstring of its binding module states.  `sources` and `headers` are relative to csrc/, `headers`
being every file the sources reach through quoted #includes; `binding` names the ctypes module of ubresnet_amd that loads `out`.

The shared libraries have NO PyTorch dependency: they are plain HIP behind the public headers in include/.  Objects are compiled
in parallel, one per translation unit, with the same flags.  source_hash() covers the network's library only.

EXTRAS and ADDONS are two more tables of the same tuples, for libraries whose sources live under csrc/extra/: build_extras() and
build_addons() build them with the same compiler, flags and commands; on the command line `--addons` and `--extras` build them
after LIBS, ADDONS first.  (Why there are three tables: DESIGN.md, "Three build tables".)
"""
from collections import namedtuple
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libubresnet_hip.so")
SOURCES = ["ubr_conv.hip", "ubr_aspp.hip", "ubr_wgrad.hip", "ubr_elem.hip", "ubr_head.hip", "ubr_tape.hip"]
HEADERS = ["ubr_common.h", "ubr_conv_epi.h", "ubr_host.h", os.path.join("..", "..", "include", "ubresnet_hip.h")]
Lib = namedtuple("Lib", "out sources headers binding")


def _satellite(name, *csrc_headers):
    """every satellite source includes ubr_sat.h and its public header; `csrc_headers` are the other headers of csrc/ it reaches"""
    return Lib(os.path.join(HERE, "libubresnet_%s.so" % name), ["ubr_%s.hip" % name],
               ["ubr_sat.h"] + list(csrc_headers) + [os.path.join("..", "..", "include", "ubresnet_%s.h" % name)], "_" + name)


LIBS = {
    "hip": Lib(OUT, SOURCES, HEADERS, "_lib"),
    "post": _satellite("post"),
    "data": _satellite("data"),
    "aug": _satellite("aug"),
    "opt": _satellite("opt", "ubr_opt_rule.h"),
    "weight": _satellite("weight", "ubr_weight_tile.h"),
    "group": _satellite("group", "ubr_group_plan.h", "ubr_opt_rule.h"),
    "ema": _satellite("ema", "ubr_ema_sched.h"),
    "accum": _satellite("accum"),
    "stats": _satellite("stats", "ubr_stats_decide.h"),
    "loss": _satellite("loss", "ubr_loss_term.h", "ubr_rows.h"),
    "dice": _satellite("dice", "ubr_dice_term.h", "ubr_rows.h"),
    "tta": _satellite("tta"),
    "det": _satellite("det", "ubr_det_rule.h"),
}

EXTRAS = {
    "score": Lib(os.path.join(HERE, "libubresnet_score.so"), [os.path.join("extra", "ubr_score.hip")],
                 ["ubr_sat.h", "ubr_wave.h", os.path.join("..", "..", "include", "ubresnet_score.h")], "_score"),
}

# the libraries after EXTRAS join this table: its tests pin what it contains, not its length
ADDONS = {
    "blend": Lib(os.path.join(HERE, "libubresnet_blend.so"), [os.path.join("extra", "ubr_blend.hip")],
                 ["ubr_sat.h", os.path.join("..", "..", "include", "ubresnet_blend.h")], "_blend"),
    "sparse": Lib(os.path.join(HERE, "libubresnet_sparse.so"), [os.path.join("extra", "ubr_sparse.hip")],
                  ["ubr_sat.h", "ubr_sparse_plan.h", "ubr_scan_plan.h", "ubr_wave.h", os.path.join("..", "..", "include", "ubresnet_sparse.h")], "_sparse"),
    "crop": Lib(os.path.join(HERE, "libubresnet_crop.so"), [os.path.join("extra", "ubr_crop.hip")],
                ["ubr_sat.h", "ubr_crop_rule.h", "ubr_det_rule.h", "ubr_wave.h", os.path.join("..", "..", "include", "ubresnet_crop.h"),
                 os.path.join("..", "..", "include", "ubresnet_det.h")], "_crop"),
    "calib": Lib(os.path.join(HERE, "libubresnet_calib.so"), [os.path.join("extra", "ubr_calib.hip")],
                 ["ubr_sat.h", "ubr_calib_plan.h", os.path.join("..", "..", "include", "ubresnet_calib.h")], "_calib"),
    "cluster": Lib(os.path.join(HERE, "libubresnet_cluster.so"), [os.path.join("extra", "ubr_cluster.hip")],
                   ["ubr_sat.h", "ubr_cluster_plan.h", "ubr_scan_plan.h", "ubr_wave.h", os.path.join("..", "..", "include", "ubresnet_cluster.h")], "_cluster"),
    "moment": Lib(os.path.join(HERE, "libubresnet_moment.so"), [os.path.join("extra", "ubr_moment.hip")],
                  ["ubr_sat.h", "ubr_moment_plan.h", "ubr_scan_plan.h", "ubr_walk_plan.h", "ubr_adc_rule.h", "ubr_walk.h", "ubr_wave.h",
                   os.path.join("..", "..", "include", "ubresnet_moment.h")], "_moment"),
    "overlap": Lib(os.path.join(HERE, "libubresnet_overlap.so"), [os.path.join("extra", "ubr_overlap.hip")],
                   ["ubr_sat.h", "ubr_overlap_plan.h", "ubr_scan_plan.h", "ubr_walk_plan.h", "ubr_adc_rule.h", "ubr_walk.h", "ubr_wave.h",
                    os.path.join("..", "..", "include", "ubresnet_overlap.h")], "_overlap"),
    "match": Lib(os.path.join(HERE, "libubresnet_match.so"), [os.path.join("extra", "ubr_match.hip")],
                 ["ubr_sat.h", "ubr_match_plan.h", "ubr_scan_plan.h", "ubr_walk_plan.h", "ubr_adc_rule.h", "ubr_walk.h", "ubr_wave.h",
                  os.path.join("..", "..", "include", "ubresnet_match.h")], "_match"),
}


def __getattr__(name):
    """POST_OUT .. DET_OUT were public constants of this module; they read LIBS[name].out, so that code outside this tree that
    imports them (the suite of an earlier commit run against this build reads them at import) keeps loading.  New code uses LIBS."""
    if name.endswith("_OUT") and name[:-4].lower() in LIBS:
        return LIBS[name[:-4].lower()].out
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
         "-fno-gpu-rdc", "-ffp-contract=off"]


def source_hash():
    """sha256 over the kernel sources and headers: stamps measurement files that are only valid for one build of the kernels"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SOURCES) + sorted(HEADERS):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _build(table, what, force, verbose, only, echo):
    """compile what is out of date and link every library of `table`, or those named in `only`; -> their paths, in table order"""
    unknown = [n for n in only or () if n not in table]
    if unknown:
        raise ValueError("%s: no library named %s; the libraries are %s" % (what, unknown, list(table)))
    libs = [lib for name, lib in table.items() if only is None or name in only]
    jobs, links = [], []
    for out, sources, headers, _ in libs:
        hdrs = [os.path.join(CSRC, h) for h in headers]
        objs, stale = [], False
        for s in sources:
            src = os.path.join(CSRC, s)
            obj = os.path.join(CSRC, s.replace(".hip", ".o"))
            objs.append(obj)
            if force or not _newer(obj, [src] + hdrs):
                jobs.append([HIPCC] + FLAGS + ["-c", src, "-o", obj])
                stale = True
        links.append((out, objs, stale))

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=echo(), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        return cmd, r

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            for cmd, r in ex.map(run, jobs):
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    raise RuntimeError("hipcc failed: " + " ".join(cmd))
                if verbose and r.stderr.strip():
                    sys.stderr.write(r.stderr)
    for out, objs, stale in links:
        if stale or force or not _newer(out, objs):
            cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
            cmd, r = run(cmd)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise RuntimeError("link failed")
    return [lib.out for lib in libs]


def build(force=False, verbose=True, only=None):
    """compile what is out of date and link every library of LIBS, or those named in `only`; -> their paths, in table order"""
    return _build(LIBS, "build", force, verbose, only, lambda: sys.stdout)


def build_extras(force=False, verbose=True, only=None):
    """the same for EXTRAS; the commands are echoed to stderr, so that a caller's stdout carries what it carried before EXTRAS"""
    return _build(EXTRAS, "build_extras", force, verbose, only, lambda: sys.stderr)


def build_addons(force=False, verbose=True, only=None):
    """the same for ADDONS; echoed to stderr as well"""
    return _build(ADDONS, "build_addons", force, verbose, only, lambda: sys.stderr)


if __name__ == "__main__":
    paths = build(force="--force" in sys.argv)
    if "--addons" in sys.argv:
        paths += build_addons(force="--force" in sys.argv)
    if "--extras" in sys.argv:
        paths += build_extras(force="--force" in sys.argv)
    print("\n".join(paths))
