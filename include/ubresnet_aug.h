/*
 * ubresnet_aug.h -- C ABI of libubresnet_aug.so (device-side augmentation of training batches: zero-pad, flip and crop per
 * image, fused with the label conversion of the loader; gfx950 / MI355X).
 *
 * A fourth, small library next to libubresnet_hip.so (include/ubresnet_hip.h), libubresnet_post.so (include/ubresnet_post.h)
 * and libubresnet_data.so (include/ubresnet_data.h).  It links against none of them and shares no state with them: it has its
 * own per-thread error string and its one launch is a plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_data.h: device pointers unless stated, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host before any launch, 0 on success or a negative UBA_E* code with a message in
 * uba_last_error().  No function allocates, frees or synchronises.
 */
#ifndef UBRESNET_AUG_H
#define UBRESNET_AUG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBA_OK 0
#define UBA_EINVAL (-1)   /* bad argument */
#define UBA_ELAUNCH (-2)  /* hip launch error */

/* launch geometry of uba_augment_batch (tests derive their sizes from it): a lane takes UBA_LANE_PIXELS consecutive output
 * columns of one row, with all planes, per trip; a row is ceil(W / UBA_LANE_PIXELS) such groups (the last one may be partial)
 * and the batch B*H*ceil(W / UBA_LANE_PIXELS) groups; a workgroup has UBA_BLOCK lanes; the grid is
 * min(ceil(groups / UBA_BLOCK), UBA_MAX_GRID) workgroups and strides over the rest. */
#define UBA_LANE_PIXELS 4
#define UBA_BLOCK 256
#define UBA_MAX_GRID 1024

#define UBA_MAX_BATCH 256   /* the per-image parameters travel by value in the kernel's arguments, one 32-bit word each */
#define UBA_MAX_PAD 16383   /* an offset (0..2*pad) has 15 bits of that word */

/* padandcropandflip (training/train_ubresnet2018_wlarcv1.py:59-68) on image, label and weight at once, out of place, in one
 * launch, fused with what ubd_prep_batch does to the batch as it came off the wire.
 *
 *   image          [B][P][H][W] fp32, read
 *   label_wire     [B][H][W] fp32, the labels as the loader delivers them, read
 *   weight         [B][H][W] fp32, read; or NULL: the wire had no weights, every source weight is 1.0f
 *   image_out      [B][P][H][W] fp32, written
 *   label_out      [B][H][W] int64, written
 *   weight_out     [B][H][W] fp32, written
 *   B, P, H, W     all >= 1; B <= UBA_MAX_BATCH; B*H*W < 2^31
 *   pad            0 <= pad <= UBA_MAX_PAD: each image is padded by `pad` pixels on every side before it is flipped and cut
 *   params         HOST array [B][4] int32: (flip_rows, flip_cols, off_r, off_c) of image b; flips in {0, 1},
 *                  0 <= off <= 2*pad.  Read during the call only.
 *   label_offset, use_threshold, threshold      as ubd_prep_batch takes them
 *   pad_label      label of a pixel cut from the padding
 *   pad_weight     weight of a pixel cut from the padding
 *
 * Output pixel (b, r, c):
 *   pr = r + off_r;  if flip_rows: pr = (H + 2*pad - 1) - pr;  sr = pr - pad
 *   pc = c + off_c;  if flip_cols: pc = (W + 2*pad - 1) - pc;  sc = pc - pad
 *   inside (0 <= sr < H and 0 <= sc < W):
 *     image_out[b][p][r][c] = T(image[b][p][sr][sc])    for every plane p
 *     label_out[b][r][c]    = L(label_wire[b][sr][sc])
 *     weight_out[b][r][c]   = weight ? weight[b][sr][sc] : 1.0f
 *   outside:
 *     image_out = +0.0f, label_out = pad_label, weight_out = pad_weight
 *
 * T and L are the per-pixel rules of ubd_prep_batch (include/ubresnet_data.h).  L, for v = label_wire[..]:
 *   |v| < 2^31          (int64) trunc(v) + label_offset     (toward zero: -0.0 and subnormals give label_offset)
 *   otherwise           INT64_MIN                           (NaN and the infinities included)
 * With the threshold on, decided on the ORIGINAL image values (x < threshold, strict: a NaN is not below):
 *   T(x) = +0.0f where x is below the threshold, x elsewhere; L = 0 for a pixel whose P values are all below.
 * With the threshold off T(x) = x, bit for bit.
 * So the result is the geometric transform of what ubd_prep_batch would have produced.
 *
 * Pointers need natural alignment only (4 bytes for float, 8 for int64_t).  When the three outputs are 16-byte aligned and
 * W % 4 == 0 a lane writes 16 bytes of image per plane, 16 of weight and 32 of labels with vector stores; otherwise it writes
 * by elements.  The sources are read by elements.  No source is written, no byte outside the three outputs is written, none
 * outside the sources is read.  No source may overlap a destination and no destination another: that is refused. */
int uba_augment_batch(const float* image, const float* label_wire, const float* weight,
                      float* image_out, int64_t* label_out, float* weight_out,
                      int B, int P, int H, int W, int pad, const int32_t* params,
                      int32_t label_offset, int use_threshold, float threshold,
                      int32_t pad_label, float pad_weight, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* uba_last_error(void);
int uba_version(void);

#ifdef __cplusplus
}
#endif

#endif
