/*
 * ubresnet_post.h -- C ABI of libubresnet_post.so (event products of whole-view inference, gfx950 / MI355X).
 *
 * A second, small library next to libubresnet_hip.so (include/ubresnet_hip.h).  It does not link against the main
 * library and shares no state with it: it has its own per-thread error string and its launches are plain <<<>>> on the
 * stream it is given (they are not recorded on a launch tape; inference replays a captured hipGraph and this call sits
 * behind the replay, where ubr_stitch_tiles sits for dense scores).
 *
 * Conventions are those of ubresnet_hip.h: device pointers unless stated, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host, 0 on success or a negative UBP_E* code with a message in ubp_last_error().
 * No function allocates, frees or synchronises.
 */
#ifndef UBRESNET_POST_H
#define UBRESNET_POST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBP_OK 0
#define UBP_EINVAL (-1)   /* bad argument */
#define UBP_ELAUNCH (-2)  /* hip launch error */

#define UBP_MAX_TILES 64    /* tile descriptors per call (UBR_MAX_TILES of ubr_stitch_tiles) */
#define UBP_MAX_CLASSES 16

/* Stitch per-tile log-probabilities into event products: a class per pixel, its probability as an IEEE half, and a
 * per-plane histogram of the classes -- only where the wire signal is above threshold.  What the reference's deploy loops
 * obtain on the host from dense scores (deploy/run_ubresnet_precropped.py:157, then argmax / exp and the blanking of
 * tf/compare_caffe_to_tf.py:17,81-89, ADC_THRESHOLD = 10.0).
 *
 *   logp            [ntiles][C][th][tw] fp32 log-probabilities, 1 <= C <= UBP_MAX_CLASSES
 *   tile_desc_host  HOST pointer, ntiles x 7 int32 {plane, row0, col0, keep_r0, keep_r1, keep_c0, keep_c1}: the tile's origin
 *                   in the view and its keep window [keep_r0, keep_r1) x [keep_c0, keep_c1) in tile coordinates, as
 *                   ubr_stitch_tiles takes them; 1 <= ntiles <= UBP_MAX_TILES, 0 <= plane < P, the origin inside the view,
 *                   the keep window inside the tile
 *   adc             [P*vplanes][rows][cols] fp32, or NULL: every pixel is lit; vplanes >= 1
 *   label           [P][rows][cols] uint8
 *   confidence      [P][rows][cols] IEEE half bits
 *   counts          [P][C] or NULL; ADDED to
 *   fill_label      0..255
 *
 * Every pixel (plane, oy, ox) inside a tile's keep window and inside the view is written by that tile:
 *   lit    <=> adc == NULL, or max over v < vplanes of adc[plane*vplanes + v][oy][ox] > adc_threshold (strict; NaN is not lit)
 *   lit:   label = the first arg-max over the classes (start at class 0, replace on a strictly greater value: a NaN in
 *          class 0 keeps label 0, a NaN elsewhere never wins); confidence = half(expf(logp[label])), round to nearest even,
 *          subnormals kept, overflow to +inf, NaN stays NaN; counts[plane][label] += 1
 *   unlit: label = fill_label, confidence = +0, nothing counted, the pixel's scores are not read
 * Bytes outside every keep window, or outside the view, are not written. */
int ubp_stitch_products(const float* logp, int C, int th, int tw, const int32_t* tile_desc_host, int ntiles,
                        const float* adc, int vplanes, float adc_threshold,
                        uint8_t* label, uint16_t* confidence, unsigned long long* counts,
                        int fill_label, int P, int rows, int cols, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubp_last_error(void);
int ubp_version(void);

#ifdef __cplusplus
}
#endif

#endif
