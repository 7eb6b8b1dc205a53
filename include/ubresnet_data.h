/*
 * ubresnet_data.h -- C ABI of libubresnet_data.so (device-side batch preparation of the training loader, gfx950 / MI355X).
 *
 * A third, small library next to libubresnet_hip.so (include/ubresnet_hip.h) and libubresnet_post.so
 * (include/ubresnet_post.h).  It links against neither and shares no state with them: it has its own per-thread error
 * string and its launches are plain <<<>>> on the stream it is given.
 *
 * Conventions are those of ubresnet_hip.h: device pointers unless stated, `stream` is a hipStream_t passed as void*,
 * arguments are validated on the host before any launch, 0 on success or a negative UBD_E* code with a message in
 * ubd_last_error().  No function allocates, frees or synchronises.
 */
#ifndef UBRESNET_DATA_H
#define UBRESNET_DATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UBD_OK 0
#define UBD_EINVAL (-1)   /* bad argument */
#define UBD_ELAUNCH (-2)  /* hip launch error */

/* launch geometry of ubd_prep_batch (tests derive their pixel counts from it): a lane takes UBD_LANE_PIXELS consecutive
 * pixels per trip, a workgroup has UBD_BLOCK lanes, the grid is min(ceil(n / (UBD_BLOCK * UBD_LANE_PIXELS)), UBD_MAX_GRID)
 * workgroups and strides over the rest. */
#define UBD_LANE_PIXELS 4
#define UBD_BLOCK 256
#define UBD_MAX_GRID 2048

/* What prep_data (training/train_ubresnet2018_wlarcv2.py:576-615) does on the host between loader[0] and the tensors it
 * returns, in one launch on the batch as it came off the wire.
 *
 *   label_wire     [n] fp32, the labels as the loader delivers them
 *   label          [n] int64, written
 *   n              pixels of the batch, B*H*W; 1 <= n < 2^31
 *   label_offset   added to every converted label: 0 for the larcv2 driver, -1 for larcv1_interface.py:59
 *   image          [B][planes][hw] fp32, updated in place -- read and written ONLY when use_threshold != 0, else it may be NULL
 *   planes, hw     planes >= 1; with use_threshold != 0 also hw >= 1 and n a multiple of hw (hw = H*W)
 *   use_threshold  0: off (prep_data's lines :607-609 are commented out in the reference), else on
 *   threshold      the ADC threshold
 *   weight_fill    [n] fp32 or NULL.  Not NULL: every weight becomes 1.0f (the wire had no weight entry, :604-605).
 *                  NULL: no weight is touched.
 *
 * Label of pixel i, v = label_wire[i]:
 *   |v| < 2^31          (int64) trunc(v) + label_offset     (toward zero, as astype(np.int): -0.0 and subnormals give label_offset)
 *   otherwise           INT64_MIN                           (NaN and the infinities included; PixelWiseNLLLoss reports it
 *                                                            as an out-of-range label, it is not ignore_index)
 * With the threshold on, decided on the ORIGINAL image values (x < threshold, strict: a NaN is not below):
 *   every image element below the threshold becomes +0.0f
 *   the label of a pixel whose `planes` values are all below becomes 0
 *
 * Pointers need natural alignment only (4 bytes for float, 8 for int64_t).  A region that is 16-byte aligned is read with
 * 16-byte loads and written with 32 bytes per lane; any other with element accesses.  No byte outside label[0..n),
 * weight_fill[0..n) and, with the threshold on, image[0..n*planes) is written, and none outside the inputs is read. */
int ubd_prep_batch(const float* label_wire, int64_t* label, int64_t n, int32_t label_offset,
                   float* image, int planes, int64_t hw, int use_threshold, float threshold,
                   float* weight_fill, void* stream);

/* message of the calling thread's last failed call ("" if none) */
const char* ubd_last_error(void);
int ubd_version(void);

#ifdef __cplusplus
}
#endif

#endif
