// ingest_bench.hip — k_ingest (csrc/jmh_ingest.hip) against its yardstick, a device-to-device
// hipMemcpyAsync of the packed picture's bytes: the kernel moves the same bytes once, with at most a
// shuffle or a shift.  HIP events around each, alternating, on one stream.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I h264-jm-commentary_amd/csrc -I include tools/ingest_bench.hip \
//         -L h264-jm-commentary_amd/csrc -ljmhip -Wl,-rpath,'$ORIGIN/../h264-jm-commentary_amd/csrc' -o tools/ingest_bench_bin
//   tools/ingest_bench_bin [reps]
// The sources are tight planes in one allocation (16-byte aligned: the 16-byte loads); a second row
// per shape offsets every plane by 2 bytes (the dword loads with v_alignbyte).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "jmh_launch.h"
#include "jmh_ingest.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static float median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static void shape(const char *name, int format, int w, int h, int bd, int mis, int reps, hipStream_t st) {
    const int W = (w + 15) / 16 * 16, H = (h + 15) / 16 * 16, es = jmi_wide(format) ? 2 : 1;
    const size_t fsize = (size_t)W * H * 3 / 2 * es;
    uint8_t *src, *dst, *cpy;
    unsigned long long *clamped;
    CK(hipMalloc(&src, fsize + 4096)); CK(hipMalloc(&dst, fsize)); CK(hipMalloc(&cpy, fsize)); CK(hipMalloc(&clamped, 8));
    CK(hipMemset(src, 1, fsize + 4096));                       // 16-bit samples 0x0101 = 257 <= maxv; nothing clamps
    CK(hipMemset(clamped, 0, 8));
    IngestArgs a;
    size_t off = mis;
    for (int sp = 0; sp < 3; sp++) {
        a.plane[sp] = sp < jmi_planes(format) ? src + off : nullptr;
        a.stride[sp] = sp < jmi_planes(format) ? jmi_row_bytes(format, sp, w) : 0;
        if (sp < jmi_planes(format)) off += ((size_t)a.stride[sp] * jmi_rows(sp, h) + 255) / 256 * 256;
    }
    a.dst = dst; a.w = w; a.h = h; a.W = W; a.H = H; a.maxv = (1u << bd) - 1; a.clamped = clamped;
    hipEvent_t e[4];
    for (auto &x : e) CK(hipEventCreate(&x));
    std::vector<float> tk, tc;
    for (int r = 0; r < reps + 10; r++) {
        CK(hipEventRecord(e[0], st));
        CK(jmh_launch_ingest(format, a, st));
        CK(hipEventRecord(e[1], st));
        CK(hipEventRecord(e[2], st));
        CK(hipMemcpyAsync(cpy, dst, fsize, hipMemcpyDeviceToDevice, st));
        CK(hipEventRecord(e[3], st));
        CK(hipStreamSynchronize(st));
        float a_ms, b_ms;
        CK(hipEventElapsedTime(&a_ms, e[0], e[1])); CK(hipEventElapsedTime(&b_ms, e[2], e[3]));
        if (r >= 10) { tk.push_back(a_ms); tc.push_back(b_ms); }   // the first ten warm up
    }
    const float k = median(tk), c = median(tc);
    printf("%-11s %4dx%-4d in %4dx%-4d base+%d  %9zu bytes  k_ingest %7.1f us (min %7.1f)  copy D2D %7.1f us (min %7.1f)  ratio %.2f  %6.1f GB/s written\n",
           name, w, h, W, H, mis, fsize, 1e3 * k, 1e3 * *std::min_element(tk.begin(), tk.end()), 1e3 * c,
           1e3 * *std::min_element(tc.begin(), tc.end()), k / c, fsize / (k * 1e-3) / 1e9);
    for (auto &x : e) CK(hipEventDestroy(x));
    CK(hipFree(src)); CK(hipFree(dst)); CK(hipFree(cpy)); CK(hipFree(clamped));
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    printf("k_ingest against hipMemcpyAsync D2D of the packed picture, HIP events, alternating, median of %d\n", reps);
    for (int mis = 0; mis <= 2; mis += 2) {
        shape("1080p I420", JMI_I420, 1920, 1080, 8, mis, reps, st);
        shape("1080p NV12", JMI_NV12, 1920, 1080, 8, mis, reps, st);
        shape("2160p I010", JMI_I010, 3840, 2160, 10, mis, reps, st);
        shape("2160p P010", JMI_P010, 3840, 2160, 10, mis, reps, st);
    }
    CK(hipStreamDestroy(st));
    return 0;
}
