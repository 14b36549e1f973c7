/*
 * jmhip_scale.h — pictures pushed from the device resampled to a chosen size (DESIGN.md §5.11, row
 * f12): a transcoder's 2160p frame, a renderer's frame or a tensor of any even size is scaled by the
 * library to out_width x out_height and padded to the coded size, where jmhip_input.h alone takes
 * only sources of the coded size or less.  Part of the C ABI of jmhip.h (which includes this file
 * directly before jmhip_output.h).  Additive only: JMH_ABI_VERSION stays 14, no struct, enum value
 * or entry point of the other headers changes.
 *
 * The setting.  jmh_input_scale sets one sticky setting on the context (NULL, or filter
 * JMH_SCALE_OFF: off, the default).  While it is set, every device push (jmh_frame_push_device,
 * jmh_frame_push_coded_device, jmh_frame_push_tensor, jmh_frame_push_coded_tensor, with the RGB
 * formats through the _device calls) and every unit seam (jmh_ingest_picture, jmh_ingest_tensor)
 * takes a source of width x height that is even and within 2..JMH_SCALE_SRC_MAX: the coded size no
 * longer bounds it.  The source is resampled to out_width x out_height (even, 2..coded size) and the
 * result is padded to the coded size by replicating its last column and row, chroma at half size, as
 * jmhip_input.h pads.  crop_w / crop_h, the slices, the NAL heads, the pops and the ordering
 * contract of jmhip_input.h are unchanged: the scaler runs on the context's stream directly behind
 * the packing kernel.  Host pushes ignore the setting.  With the setting off every call behaves as
 * before, the size refusals included.
 *
 * Errors.  jmh_input_scale answers JMH_E_INVALID_ARG, and leaves the setting as it was, for a filter
 * outside 0..3, an unknown flag, or an output size that is odd or outside 2..coded size.  A push whose
 * source needs more than JMH_SCALE_TAPS_MAX taps on an axis (luma or chroma) answers
 * JMH_E_UNSUPPORTED_CFG with nothing claimed or queued.
 *
 * Lifetime.  The setting may change while pictures are in flight: a picture is scaled with the
 * setting that held at its push.
 *
 * Sources of every kind through one scaler.  Scaling works on the packed 4:2:0 picture, not on each
 * format: the packing kernel of the source's kind (planes, packed RGB, tensor) packs the source at
 * its own size, rounded up to multiples of 16 by its own replication, into a scratch picture the
 * context owns, and the scaler reads the width x height samples of that.  So RGB is converted and its
 * chroma boxed at source resolution, then scaled.  jmh_device_input_clamped still counts the I010
 * samples of the source.
 *
 * Arithmetic, exact integers.  Per axis, n_src samples to n_dst:
 *   r = n_src / n_dst, s = max(1, r); phi = 0.25 for the horizontal axis of the chroma planes when
 *   JMH_SCALE_CHROMA_LEFT is set, else 0.5.  Output sample i sits at c_i = (i + phi) r - phi.
 *   Kernels k(t) of support S: bilinear the triangle 1 - |t| (S = 1); bicubic Catmull-Rom, a = -0.5
 *   (S = 2); Lanczos3 sinc(t) sinc(t / 3) (S = 3); 0 outside the support.
 *   T = 2 ceil(S s) taps for every output sample of the axis (the ceiling of the exact rational);
 *   T > JMH_SCALE_TAPS_MAX is the unsupported case.  first_i = floor(c_i - T / 2) + 1, stored
 *   unclamped.  Tap j = first_i .. first_i + T - 1 has the real weight w_j = k((j - c_i) / s) and the
 *   integer weight q_j = floor(w_j / sum(w) * 16384 + 0.5); then 16384 - sum(q) is added to the first
 *   tap of largest q, so every row sums to exactly 16384.  The sample read for tap j is
 *   src[min(max(j, 0), n_src - 1)]: edge replication.  c_i, w and q are computed in IEEE double, in
 *   the order written here, the sum over ascending j.
 *   jmh_scale_taps returns exactly these tables: first[n_dst], taps[n_dst * T] row by row, *ntaps = T.
 *   With first and taps NULL it returns only *ntaps.  It guarantees sum(|q|) <= 32767 for every row.
 * Two passes, horizontal first, with P = 14 - bit depth (6, 5 or 4); >> is an arithmetic shift:
 *   h = (sum(q_j src_j) + (1 << (13 - P))) >> (14 - P)
 *   v = (sum(q_k h_k)   + (1 << (13 + P))) >> (14 + P), clamped to 0 .. maxv.
 * As maxv 2^P < 2^14, h fits an int16_t whenever sum(|q|) <= 32767, and the vertical sum stays below
 * 2^30.  U and V are scaled as planes of half size, width/2 x height/2 to out_width/2 x out_height/2.
 * Consequence: with the source size equal to the output size every row is the single tap 16384 and
 * the result is the source, byte for byte.
 */
#ifndef JMHIP_SCALE_H
#define JMHIP_SCALE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { JMH_SCALE_OFF = 0, JMH_SCALE_BILINEAR = 1, JMH_SCALE_BICUBIC = 2, JMH_SCALE_LANCZOS3 = 3 };
enum { JMH_SCALE_CHROMA_LEFT = 1 };           /* flags: 4:2:0 chroma is left-sited (MPEG-2 / H.264 default), else centred */
#define JMH_SCALE_TAPS_MAX 24
#define JMH_SCALE_SRC_MAX  8192
typedef struct jmh_scale { int32_t filter, flags, out_width, out_height; } jmh_scale;

int jmh_input_scale(jmh_ctx *ctx, const jmh_scale *s);    /* NULL or filter OFF: off (the default) */
int jmh_scale_taps(int n_src, int n_dst, int filter, int chroma_left, int32_t *first, int16_t *taps, int *ntaps);
int jmh_scale_info(const jmh_ctx *ctx, jmh_scale *s, int *active);   /* the current setting */

#ifdef __cplusplus
}
#endif
#endif /* JMHIP_SCALE_H */
