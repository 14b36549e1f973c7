// jmh_launch.h — the host-side launchers of the gfx950 kernels, one prototype each: included by the
// translation unit that defines a launcher (next to its kernels) and by the C ABI (jmhip_abi.hip).
#pragma once
#include "jmh_device.h"

// the macroblock wavefront (one launch per tick / per dataflow segment)
hipError_t jmh_launch_analyse(const TickArgs &t, hipStream_t st);                  // jmh_analyse.hip
hipError_t jmh_launch_intra(const TickArgs &t, hipStream_t st);
hipError_t jmh_launch_flow(const FlowArgs &f, hipStream_t st);                     // jmh_flow.hip
hipError_t jmh_launch_intra8(const TickArgs &t, hipStream_t st);                   // jmh_intra8.hip
hipError_t jmh_launch_me_full(const TickArgs &t, hipStream_t st);                  // jmh_fullsearch.hip
hipError_t jmh_launch_epzs(const TickArgs &t, hipStream_t st);                     // jmh_epzs.hip
hipError_t jmh_launch_final(const TickArgs &t, hipStream_t st);                    // jmh_final.hip
hipError_t jmh_launch_rdo(const TickArgs &t, hipStream_t st, hipStream_t side, hipEvent_t fork, hipEvent_t join);   // jmh_rdo.hip
size_t jmh_rdo_scratch_bytes();
hipError_t jmh_launch_ingest(int format, const IngestArgs &a, hipStream_t st);      // jmh_ingest.hip
hipError_t jmh_launch_ingest_rgb(int format, const RgbArgs &a, hipStream_t st);    // jmh_rgb.hip
hipError_t jmh_launch_ingest_yuv(int format, const YuvArgs &a, hipStream_t st);    // jmh_yuv.hip
hipError_t jmh_launch_ingest_tensor(int dtype, const TensorArgs &a, hipStream_t st);   // jmh_tensor.hip
hipError_t jmh_launch_scale(const ScaleArgs &a, hipStream_t st);                         // jmh_scale.hip
hipError_t jmh_launch_pull_picture(int format, const OutArgs &a, hipStream_t st);      // jmh_output.hip
hipError_t jmh_launch_pull_tensor(int dtype, const OutArgs &a, hipStream_t st);

// the unit seams: pel = uint8_t or uint16_t samples (instantiated for both where they are defined);
// qpb = qp + QpBdOffset, maxv = (1 << bit depth) - 1 (8 bits: qp and 255)
hipError_t jmh_launch_interp(const uint8_t *ref, int W, int H, uint8_t *qpel, int qstride, int qplane, hipStream_t st);   // jmh_kernels.hip
hipError_t jmh_launch_spiral_positions(int count, int32_t *out_xy, hipStream_t st);   // jmh_kernels.hip (jmhip_spiral.h)
template <class pel>
hipError_t jmh_launch_sad_table(const pel *org, const pel *ref, int W, int H, int sr, int n_mb, const int32_t *mb_xy, const int32_t *centres,
                                uint16_t *out, hipStream_t st);
template <class pel>
hipError_t jmh_launch_tq4x4(int n, const int16_t *resid, const pel *pred, int qpb, int qsel, int maxv, int16_t *levels, pel *recon,
                            int32_t *cc, int32_t *nz, hipStream_t st);
template <class pel>
hipError_t jmh_launch_tq8x8(int n, const int16_t *resid, const pel *pred, int qpb, int qsel, int maxv, int16_t *levels, pel *recon,
                            int32_t *cc, int32_t *nz, hipStream_t st);
template <class pel>
hipError_t jmh_launch_block_search(int n, const jmh_block_search *reqs, jmh_block_result *out, const pel *cur, const pel *ref, int W, int H,
                                   int had, int maxv, hipStream_t st);                                                     // jmh_block.hip
