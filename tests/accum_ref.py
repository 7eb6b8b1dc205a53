"""numpy replay of libubresnet_accum.so (include/ubresnet_accum.h): the three calls in np.float32 operations, element for
element, each rounded once (numpy keeps subnormals and does not contract).  The geometry is restated here so that tests hold the
header, the binding and this file against each other."""
import numpy as np

BLOCK, UNROLL, MAX_GRID = 256, 4, 1024
TRIP = BLOCK * UNROLL                    # consecutive units (of four floats) a workgroup takes per trip

f32 = np.float32


def set_(grad):
    """ubc_set: -> the accumulator, the gradient's bytes"""
    return np.asarray(grad, dtype=f32).view(np.uint32).copy().view(f32)


def add(acc, grad):
    """ubc_add: -> the new accumulator, acc + grad"""
    acc, grad = np.asarray(acc, dtype=f32), np.asarray(grad, dtype=f32)
    with np.errstate(all="ignore"):
        return (acc + grad).astype(f32)


def finish(acc, grad, scale):
    """ubc_finish: -> the new gradient, (acc + grad) * scale: the sum is rounded, then the product"""
    acc, grad = np.asarray(acc, dtype=f32), np.asarray(grad, dtype=f32)
    with np.errstate(all="ignore"):
        s = (acc + grad).astype(f32)
        return (s * f32(scale)).astype(f32)


def scale_of(every, average=True):
    """the launch argument of ubc_finish as GradAccumulator computes it"""
    return f32(1.0 / every) if average else f32(1.0)


def cycle(grads, scale):
    """a whole cycle over the micro-batch gradients `grads` (two or more): set, add .., finish -> what the flat gradient holds"""
    assert len(grads) >= 2
    acc = set_(grads[0])
    for g in grads[1:-1]:
        acc = add(acc, g)
    return finish(acc, grads[-1], scale)


def flat_sizes():
    """float counts n from the geometry: one unit; a workgroup's trip less one unit, exactly, plus one unit (a second workgroup
    with one unit); one trip of the whole grid at the grid cap plus one unit (workgroup 0 makes a second trip, of one unit)"""
    return [4, 4 * (TRIP - 1), 4 * TRIP, 4 * (TRIP + 1), 4 * (MAX_GRID * TRIP + 1)]


def grid(n):
    units = n // 4
    return min((units + TRIP - 1) // TRIP, MAX_GRID)
