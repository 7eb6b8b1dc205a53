/*
 * ubresnet_det.h -- C ABI of libubresnet_det.so (detector effects on a prepared training batch, in place on the device: dead
 * wires, a gain per plane and electronics noise on the image, with the label and the weight of a pixel whose wire is dead in
 * every plane; gfx950 / MI355X).
 *
 * A fourteenth, small library next to libubresnet_hip.so, libubresnet_post.so, libubresnet_data.so, libubresnet_aug.so
 * (include/ubresnet_aug.h) and the others.  It links against none of them and shares no state with them: it has its own
 * per-thread error string and its one launch is a plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_aug.h: device pointers unless stated, `stream` is a hipStream_t passed as void*, arguments
 * are validated on the host before any launch, 0 on success or a negative UBX_E* code with a message in ubx_last_error().  No
 * function allocates, frees or synchronises.
 */
#ifndef UBRESNET_DET_H
#define UBRESNET_DET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBX_OK 0
#define UBX_EINVAL (-1)   /* bad argument */
#define UBX_ELAUNCH (-2)  /* hip launch error */

/* launch geometry of ubx_apply (tests derive their sizes from it), that of uba_augment_batch: a lane takes UBX_LANE_PIXELS
 * consecutive columns of one row, with all planes, per trip; a row is ceil(W / UBX_LANE_PIXELS) such groups (the last one may be
 * partial) and the batch B*H*ceil(W / UBX_LANE_PIXELS) groups; a workgroup has UBX_BLOCK lanes; the grid is
 * min(ceil(groups / UBX_BLOCK), UBX_MAX_GRID) workgroups and strides over the rest. */
#define UBX_LANE_PIXELS 4
#define UBX_BLOCK 256
#define UBX_MAX_GRID 1024

/* the fourth counter word of every Philox call ("UBXD"): keeps the noise apart from any other use of the same key */
#define UBX_PHILOX_TAG 0x55425844u

/* Detector effects on a prepared batch -- what ubd_prep_batch or uba_augment_batch left behind -- in place, in one launch.
 *
 *   image          [B][P][H][W] fp32, read and written
 *   label          [B][H][W] int64, written where stated below; may be NULL if !set_label
 *   weight         [B][H][W] fp32, written where stated below; may be NULL if !set_weight
 *   B, P, H, W     all >= 1; B*H*W < 2^31
 *   table          DEVICE array [B][P][1 + ceil(W/32)] uint32, read.  Row (b, p): word 0 holds the bits of an fp32 gain; then
 *                  ceil(W/32) mask words: bit (c & 31) of word (c >> 5) set means column c of plane p of image b is a dead
 *                  wire.  Bits at or beyond W are ignored.
 *                  THE KERNEL TRUSTS THE TABLE: it lives on the device, so the host cannot look at it without a copy and a
 *                  wait, and this call makes neither.  Any bit pattern is a valid gain and a valid mask, so a wrong table
 *                  gives wrong pixels, never an access outside the three arrays; a table SHORTER than B*P*(1 + ceil(W/32))
 *                  words is read past its end.
 *   sigma          finite, >= 0: standard deviation of the noise; 0 switches the noise off and no random number is made
 *   noise_all      0: only lit pixels (x != 0; a NaN counts as lit) get noise; otherwise every live pixel does
 *   seed, seq      the Philox key
 *   set_label, dead_label      if set_label: label = dead_label where column c is dead in EVERY plane of image b
 *   set_weight, dead_weight    if set_weight: weight = dead_weight there; dead_weight finite
 *
 * Per element (b, p, r, c), x the value found, by the inline functions of ubresnet_amd/csrc/ubr_det_rule.h:
 *   1. column c dead in (b, p):   +0.0f
 *   2. otherwise  y = x if the gain's bits are those of 1.0f (no multiply: bit for bit, NaN payloads, -0.0f and subnormals
 *      kept), else y = __fmul_rn(x, gain)
 *   3. if sigma > 0 and (noise_all or x != 0):  y = __fadd_rn(y, __fmul_rn(sigma, z))
 * Everywhere else -- the label and the weight of a pixel with a live wire in some plane above all -- not a byte is written.
 * A lane whose four columns have no dead wire, a unit gain and no noise to add skips its store; a lane that stores writes back
 * the bytes it read where the rule leaves a value alone.
 *
 * z is a standard normal that depends on (seed, seq, b, p, r, c) alone -- not on the grid, the alignment or the vector width:
 *   (w0, w1, w2, w3) = Philox4x32-10, key (seed, seq), counter (c >> 2, r, b * P + p, UBX_PHILOX_TAG); multipliers 0xD2511F53
 *   and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85
 *   columns with c & 3 in {0, 1} use the pair (a, b') = (w0, w1), those with c & 3 in {2, 3} the pair (w2, w3)
 *   u1 = ((a >> 8) + 1) * 2^-24 in (0, 1],  u2 = (b' >> 8) * 2^-24 in [0, 1)   (both exact in fp32)
 *   rad = __fsqrt_rn(__fmul_rn(-2.0f, logf(u1)))
 *   even column: z = __fmul_rn(rad, cospif(2 u2));  odd column: z = __fmul_rn(rad, sinpif(2 u2))
 * with the accurate library functions; |z| <= sqrt(48 ln 2) ~ 5.77.  Nothing is contracted (-ffp-contract=off).
 *
 * Kernels: detector_kernel<false> is launched when sigma == 0 (dead wires and gain: no random number, no library call),
 * detector_kernel<true> when sigma > 0.
 *
 * Pointers need natural alignment only (4 bytes for float and uint32, 8 for int64_t).  When image is 16-byte aligned and
 * W % 4 == 0 a lane loads and stores 16 bytes of image per plane; otherwise it works by elements; the choice is the same for
 * the whole launch and does not change a value.  Labels and weights are stored by elements.  image, label, weight and table
 * must not overlap: that is refused. */
int ubx_apply(float* image, int64_t* label, float* weight, int B, int P, int H, int W, const uint32_t* table,
              float sigma, int noise_all, uint32_t seed, uint32_t seq,
              int set_label, int64_t dead_label, int set_weight, float dead_weight, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubx_last_error(void);
int ubx_version(void);

#ifdef __cplusplus
}
#endif

#endif
