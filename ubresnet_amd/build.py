"""Build libubresnet_hip.so (all HIP kernels of the network + the C ABI), libubresnet_post.so (event products of
whole-view inference), libubresnet_data.so (device-side batch preparation of the loader), libubresnet_aug.so (device-side
augmentation of training batches), libubresnet_opt.so (the guarded flat optimizer step), libubresnet_weight.so (device-side
pixel weights of the loss), libubresnet_group.so (flat optimizer steps with parameter groups), libubresnet_ema.so (the
exponential moving average of the parameters), libubresnet_accum.so (gradient accumulation over the flat gradient buffer),
libubresnet_stats.so (the guard of the BatchNorm running statistics), libubresnet_loss.so (the pixel-wise focal loss and its
normalised means), libubresnet_dice.so (the soft Dice / Tversky region loss), libubresnet_tta.so (flip test-time augmentation
of inference) and libubresnet_det.so (detector effects on training batches), the latter thirteen self-contained libraries of
their own, with hipcc for gfx950, in-tree.

    python -m ubresnet_amd.build [--force]

The shared libraries have NO PyTorch dependency: they are plain HIP behind include/ubresnet_hip.h,
include/ubresnet_post.h, include/ubresnet_data.h, include/ubresnet_aug.h, include/ubresnet_opt.h, include/ubresnet_weight.h, include/ubresnet_group.h, include/ubresnet_ema.h, include/ubresnet_accum.h, include/ubresnet_stats.h, include/ubresnet_loss.h, include/ubresnet_dice.h, include/ubresnet_tta.h and include/ubresnet_det.h.  Objects are compiled in parallel, one per translation unit, with the same flags.

build() makes the first nine, build_stats() the tenth, build_loss() the eleventh, build_dice() the twelfth, build_tta() the
thirteenth and build_det() the fourteenth by the same steps; the command line and the driver entry point call all six.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libubresnet_hip.so")
SOURCES = ["ubr_conv.hip", "ubr_aspp.hip", "ubr_wgrad.hip", "ubr_elem.hip", "ubr_head.hip", "ubr_tape.hip"]
HEADERS = ["ubr_common.h", "ubr_host.h", os.path.join("..", "..", "include", "ubresnet_hip.h")]
# the second library: not linked against the first; source_hash() covers the network sources only
POST_OUT = os.path.join(HERE, "libubresnet_post.so")
POST_SOURCES = ["ubr_post.hip"]
POST_HEADERS = [os.path.join("..", "..", "include", "ubresnet_post.h")]
# the third library: like the second, it links against neither of the others
DATA_OUT = os.path.join(HERE, "libubresnet_data.so")
DATA_SOURCES = ["ubr_data.hip"]
DATA_HEADERS = [os.path.join("..", "..", "include", "ubresnet_data.h")]
# the fourth library: it links against none of the others either
AUG_OUT = os.path.join(HERE, "libubresnet_aug.so")
AUG_SOURCES = ["ubr_aug.hip"]
AUG_HEADERS = [os.path.join("..", "..", "include", "ubresnet_aug.h")]
# the fifth library: it links against none of the others either
OPT_OUT = os.path.join(HERE, "libubresnet_opt.so")
OPT_SOURCES = ["ubr_opt.hip"]
OPT_HEADERS = [os.path.join("..", "..", "include", "ubresnet_opt.h")]
# the sixth library: it links against none of the others either
WEIGHT_OUT = os.path.join(HERE, "libubresnet_weight.so")
WEIGHT_SOURCES = ["ubr_weight.hip"]
WEIGHT_HEADERS = ["ubr_weight_tile.h", os.path.join("..", "..", "include", "ubresnet_weight.h")]
# the seventh library: it links against none of the others either
GROUP_OUT = os.path.join(HERE, "libubresnet_group.so")
GROUP_SOURCES = ["ubr_group.hip"]
GROUP_HEADERS = ["ubr_group_plan.h", os.path.join("..", "..", "include", "ubresnet_group.h")]
# the eighth library: it links against none of the others either
EMA_OUT = os.path.join(HERE, "libubresnet_ema.so")
EMA_SOURCES = ["ubr_ema.hip"]
EMA_HEADERS = ["ubr_ema_sched.h", os.path.join("..", "..", "include", "ubresnet_ema.h")]
# the ninth library: it links against none of the others either
ACCUM_OUT = os.path.join(HERE, "libubresnet_accum.so")
ACCUM_SOURCES = ["ubr_accum.hip"]
ACCUM_HEADERS = [os.path.join("..", "..", "include", "ubresnet_accum.h")]
# the tenth library: it links against none of the others either
STATS_OUT = os.path.join(HERE, "libubresnet_stats.so")
STATS_SOURCES = ["ubr_stats.hip"]
STATS_HEADERS = ["ubr_stats_decide.h", os.path.join("..", "..", "include", "ubresnet_stats.h")]
# the eleventh library: it links against none of the others either
LOSS_OUT = os.path.join(HERE, "libubresnet_loss.so")
LOSS_SOURCES = ["ubr_loss.hip"]
LOSS_HEADERS = ["ubr_loss_term.h", os.path.join("..", "..", "include", "ubresnet_loss.h")]
# the twelfth library: it links against none of the others either
DICE_OUT = os.path.join(HERE, "libubresnet_dice.so")
DICE_SOURCES = ["ubr_dice.hip"]
DICE_HEADERS = ["ubr_dice_term.h", os.path.join("..", "..", "include", "ubresnet_dice.h")]
# the thirteenth library: it links against none of the others either
TTA_OUT = os.path.join(HERE, "libubresnet_tta.so")
TTA_SOURCES = ["ubr_tta.hip"]
TTA_HEADERS = [os.path.join("..", "..", "include", "ubresnet_tta.h")]
# the fourteenth library: it links against none of the others either
DET_OUT = os.path.join(HERE, "libubresnet_det.so")
DET_SOURCES = ["ubr_det.hip"]
DET_HEADERS = ["ubr_det_rule.h", os.path.join("..", "..", "include", "ubresnet_det.h")]
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


def build(force=False, verbose=True):
    """compile what is out of date and link the nine libraries; -> path of the main library"""
    libs = [(OUT, SOURCES, HEADERS), (POST_OUT, POST_SOURCES, POST_HEADERS),
            (DATA_OUT, DATA_SOURCES, DATA_HEADERS), (AUG_OUT, AUG_SOURCES, AUG_HEADERS),
            (OPT_OUT, OPT_SOURCES, OPT_HEADERS), (WEIGHT_OUT, WEIGHT_SOURCES, WEIGHT_HEADERS),
            (GROUP_OUT, GROUP_SOURCES, GROUP_HEADERS), (EMA_OUT, EMA_SOURCES, EMA_HEADERS),
            (ACCUM_OUT, ACCUM_SOURCES, ACCUM_HEADERS)]
    _build(libs, force, verbose)
    return OUT


def build_stats(force=False, verbose=True):
    """the tenth library by the same steps: one more (OUT, SOURCES, HEADERS) tuple; -> its path"""
    _build([(STATS_OUT, STATS_SOURCES, STATS_HEADERS)], force, verbose)
    return STATS_OUT


def build_loss(force=False, verbose=True):
    """the eleventh library by the same steps; -> its path"""
    _build([(LOSS_OUT, LOSS_SOURCES, LOSS_HEADERS)], force, verbose)
    return LOSS_OUT


def build_dice(force=False, verbose=True):
    """the twelfth library by the same steps; -> its path"""
    _build([(DICE_OUT, DICE_SOURCES, DICE_HEADERS)], force, verbose)
    return DICE_OUT


def build_tta(force=False, verbose=True):
    """the thirteenth library by the same steps; -> its path"""
    _build([(TTA_OUT, TTA_SOURCES, TTA_HEADERS)], force, verbose)
    return TTA_OUT


def build_det(force=False, verbose=True):
    """the fourteenth library by the same steps; -> its path"""
    _build([(DET_OUT, DET_SOURCES, DET_HEADERS)], force, verbose)
    return DET_OUT


def _build(libs, force, verbose):
    jobs, links = [], []
    for out, sources, headers in libs:
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
            print(" ".join(cmd), flush=True)
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


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
    print(build_stats(force="--force" in sys.argv))
    print(build_loss(force="--force" in sys.argv))
    print(build_dice(force="--force" in sys.argv))
    print(build_tta(force="--force" in sys.argv))
    print(build_det(force="--force" in sys.argv))
