// jmh_coded.h — coded pictures (include/jmhip_coded.h): what the C ABI hands the
// slice writers when it queues a picture's writer behind the picture's last tick, and the
// distortion kernel (jmh_coded.hip) that runs behind the writer on the same stream.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/jmhip.h"

// One picture's own writer buffers (a ring entry's): nothing in them is shared with the writer of
// another picture, so several pictures' writers may be queued at once.  d_meta, eight 64-bit words,
// zeroed by the enqueue on the writer's stream:
//   [0] the picture's bytes (int64)     [1] overflow word (uint32): a counted size exceeded a capacity
//   [2..4] SSD of Y, U, V (k_plane_ssd) [5] CABAC: the picture's bins  [6] CABAC: its scratch bytes
struct jmh_writer_job {
    const void *h_sl;      // pinned: the descriptors (jmh_slice_desc / jmh_cabac_slice_desc), valid until the picture is popped
    void *d_sl;            // device: the same, uploaded by the enqueue
    void *d_where;         // device: jmh_slice_bytes / jmh_cabac_slice_bytes [n]
    uint64_t *d_meta;
    uint8_t *d_out;        // device: the picture's output region
    size_t out_cap;        // its bytes, a multiple of 4, decided before the enqueue
};
#define JMH_WRITER_META_WORDS 8
#define JMH_WRITER_META_BYTES (JMH_WRITER_META_WORDS * sizeof(uint64_t))

// ssd[pl] += sum over the crop (chroma: halved) of (a - b)^2 of two 4:2:0 pictures of W x H samples
// of ps bytes (planes contiguous: Y, U, V); one launch on st.  ssd: three zeroed 64-bit device words.
int jmh_plane_ssd(hipStream_t st, const uint8_t *a, const uint8_t *b, int W, int H, int crop_w, int crop_h, int ps, uint64_t *ssd);
