"""Reference of ubw_pixel_weights (include/ubresnet_weight.h) in numpy, written from the header's rule, the label builders its
tests share, and the table of cases that tests/test_gpu_weights_exact.py runs -- one entry per kernel compiled into
libubresnet_weight.so, which tests/test_cpu_weights.py holds against the library's symbol table.  No GPU and no torch here.

Acceptance: every output is equal to the reference bit for bit; there is no tolerance anywhere."""
import numpy as np

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
MAX_CLASSES, MAX_RADIUS = 16, 4
# launch geometry, as ubresnet_amd/csrc/ubr_weight_tile.h states it (tests/test_cpu_weights.py holds these against that file)
LANE_PIXELS, BLOCK, MAX_GRID, TILE_W, TILE_H = 4, 256, 2048, 64, 16

# the shapes (B, H, W) every radius is run at: H or W below r, widths that are no multiple of 4 or of the tile, a tile with a
# ragged last row and column, several tiles per image
GEOMETRY = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 3, 67), (3, 17, 64), (2, 33, 130), (5, 2, 3)]

# kernel (normal form of tools/kernel_symbols.py) -> ids of the cases in test_gpu_weights_exact.py that launch it.  Every call
# launches count_kernel and the apply_kernel of its radius.
KERNEL_CASES = {
    "count_kernel": ["geometry-r0", "geometry-r1", "geometry-r2", "geometry-r3", "geometry-r4", "odd-image", "classes",
                     "invalid-values", "invalid-in-window", "image-isolation", "row-isolation", "parameters", "counts-garbage",
                     "twice", "many-chunks"],
    "apply_kernel<0>": ["geometry-r0", "classes", "counts-garbage"],
    "apply_kernel<1>": ["geometry-r1", "classes", "invalid-values", "invalid-in-window", "odd-image", "twice"],
    "apply_kernel<2>": ["geometry-r2", "parameters", "row-isolation", "many-chunks"],
    "apply_kernel<3>": ["geometry-r3", "image-isolation"],
    "apply_kernel<4>": ["geometry-r4", "image-isolation", "row-isolation"],
}


def reference(label, C, max_weight=float("inf"), radius=0, gain=1.0, lo=1):
    """ubw_pixel_weights on the host.  label [B,H,W] int64 -> (weight float32 [B,H,W], counts int64 [B,16])"""
    label = np.asarray(label, np.int64)
    assert label.ndim == 3 and 1 <= C <= MAX_CLASSES and 0 <= radius <= MAX_RADIUS and 0 <= lo <= C
    B, H, W = label.shape
    weight = np.zeros((B, H, W), np.float32)
    counts = np.zeros((B, MAX_CLASSES), np.int64)
    cap = np.float64(np.float32(max_weight))
    g = np.float32(gain)
    for b in range(B):
        lab = label[b]
        valid = (lab >= 0) & (lab < C)
        n = np.bincount(lab[valid], minlength=MAX_CLASSES).astype(np.int64)
        counts[b] = n
        K, V = int((n > 0).sum()), int(n.sum())
        wc = np.zeros(MAX_CLASSES, np.float32)
        if K:
            present = n > 0
            wc[present] = np.minimum(np.float64(V) / (np.float64(K) * n[present].astype(np.float64)), cap).astype(np.float32)
        w = np.zeros((H, W), np.float32)
        w[valid] = wc[lab[valid]]
        if radius > 0:
            part = valid & (lab >= lo)                        # takes part in interfaces
            mark = np.zeros((H, W), bool)
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    # pixel (y, x) against (y + dy, x + dx), both inside the image: explicit shifted views, no wrap-around
                    ys, ye = max(0, -dy), min(H, H - dy)
                    xs, xe = max(0, -dx), min(W, W - dx)
                    if ys >= ye or xs >= xe:
                        continue
                    a, q = lab[ys:ye, xs:xe], lab[ys + dy:ye + dy, xs + dx:xe + dx]
                    mark[ys:ye, xs:xe] |= part[ys:ye, xs:xe] & part[ys + dy:ye + dy, xs + dx:xe + dx] & (a != q)
            w[mark] = w[mark] * g                              # one float32 multiply
        weight[b] = w
    return weight, counts


# ------------------------------------------------------------------------------------------------------------------------
# label builders
# ------------------------------------------------------------------------------------------------------------------------
def blobs(rs, B, H, W, C, p_other=0.25):
    """mostly class 0 with rectangles of the other classes dropped in: interfaces of every orientation, different counts per
    image, and (for C > 2) classes that an image may lack"""
    lab = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for _ in range(max(1, int(p_other * H * W / 6)) if C > 1 else 0):
            c = rs.randint(1, C)
            y, x = rs.randint(0, H), rs.randint(0, W)
            lab[b, y:y + rs.randint(1, 4), x:x + rs.randint(1, 5)] = c
        if C > 2 and b % 2 == 1:
            lab[b][lab[b] == C - 1] = 0                        # this image lacks the last class
    return lab


def noise(rs, B, H, W, C):
    """every pixel a class of its own choosing, image b drawn with its own class probabilities"""
    lab = np.zeros((B, H, W), np.int64)
    for b in range(B):
        p = rs.dirichlet(np.ones(C) * 0.7)
        lab[b] = rs.choice(C, size=(H, W), p=p)
    return lab


def invalid_values(C):
    """labels that are no class: the two below zero, the first one above, the ends of int64, and three whose LOW WORD is a
    valid class for some C (they catch a test on 32 bits)"""
    return [-1, -100, C, INT64_MIN, INT64_MAX, 2 ** 32 + 1, 2 ** 40 + 2, 2 ** 32]


def sprinkle_invalid(rs, lab, C, share=0.08):
    """`lab` with `share` of its pixels (at least one of every invalid value where the size allows) replaced by invalid values"""
    out = lab.copy().reshape(-1)
    bad = np.array(invalid_values(C), np.int64)
    k = min(out.size, max(len(bad), int(share * out.size)))
    out[rs.choice(out.size, k, replace=False)] = np.resize(bad, k)
    return out.reshape(lab.shape)
