/*
 * ubresnet_weight.h -- C ABI of libubresnet_weight.so (device-side pixel weights for PixelWiseNLLLoss: per-image class
 * balance and an interface gain, gfx950 / MI355X).
 *
 * A sixth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so and
 * libubresnet_opt.so.  It links against none of them and shares no state with them: it has its own per-thread error string
 * and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_data.h: device pointers unless stated, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host before any launch, 0 on success or a negative UBW_E* code with a message in
 * ubw_last_error().  No function allocates, frees or synchronises.
 */
#ifndef UBRESNET_WEIGHT_H
#define UBRESNET_WEIGHT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBW_OK 0
#define UBW_EINVAL (-1)   /* bad argument */
#define UBW_ELAUNCH (-2)  /* hip launch error */

#define UBW_MAX_CLASSES 16   /* columns of a row of `counts`, whatever C is */
#define UBW_MAX_RADIUS 4

/* Pixel weights of a batch of label images, two launches (a count pass and an apply pass) behind a memset of `counts`, all
 * on `stream`.
 *
 *   label        [B][H][W] int64, read only
 *   weight       [B][H][W] fp32, written
 *   counts       [B][UBW_MAX_CLASSES] int64 workspace: zeroed by the call itself, on the stream; afterwards counts[b][c] is
 *                n_c of image b for c < C and 0 for c >= C
 *   B, H, W      >= 1, B*H*W < 2^31
 *   C            classes, 1..UBW_MAX_CLASSES
 *   max_weight   cap of a class weight, > 0; +inf: no cap
 *   radius       r of the interface window, 0..UBW_MAX_RADIUS; 0 turns the gain off
 *   gain         factor of an interface pixel's weight, finite and >= 0
 *   lo           lowest class that takes part in an interface, 0..C (C: none does)
 *
 * Per image b, N = H*W:
 *   a label v is valid iff 0 <= v < C as an int64; n_c = valid pixels of class c; K = classes with n_c > 0; V = sum of n_c
 *   w_c = min((double)V / ((double)K * (double)n_c), (double)max_weight), computed in fp64 and rounded once to fp32
 *   an invalid pixel gets +0.0f
 *   a pixel with label a is an interface pixel iff lo <= a < C and some pixel of the same image in the
 *     (2r+1) x (2r+1) window around it, clipped at the image edges, has a label b with lo <= b < C and b != a
 *   an interface pixel gets fl32(w_c) * gain (one fp32 multiply), any other valid pixel fl32(w_c)
 * The counts are integers and the arithmetic is one fp64 divide, one min, one conversion and one fp32 multiply (the library
 * is built with -ffp-contract=off): every output is reproducible bit for bit.  Only integer atomics are used.
 *
 * `label` needs 8-byte and `weight` 4-byte alignment.  A region that is 16-byte aligned is accessed with 16 bytes per lane
 * (the count pass decides per image; the apply pass takes 16-byte accesses when W % 4 == 0 and the region is aligned), any
 * other with element accesses.  No byte outside weight[0..B*H*W) and counts[0..16*B) is written and none outside
 * label[0..B*H*W) is read. */
int ubw_pixel_weights(const int64_t* label, float* weight, int64_t* counts,
                      int B, int H, int W, int C,
                      float max_weight, int radius, float gain, int lo, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubw_last_error(void);
int ubw_version(void);

#ifdef __cplusplus
}
#endif

#endif
