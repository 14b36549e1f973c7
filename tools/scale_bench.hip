// scale_bench.hip — k_scale (csrc/jmh_scale.hip) against its yardstick, a device-to-device
// hipMemcpyAsync of as many bytes as the kernel has to read and write once (the source picture plus
// the destination picture).  HIP events around each, alternating, on one stream.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I h264-jm-commentary_amd/csrc -I include tools/scale_bench.hip \
//         -L h264-jm-commentary_amd/csrc -ljmhip -Wl,-rpath,'$ORIGIN/../h264-jm-commentary_amd/csrc' -o tools/scale_bench_bin
//   tools/scale_bench_bin [reps]
// The source is a packed 4:2:0 picture of the source's size rounded up to macroblocks, as the ingest
// kernels leave it; the tables are those of jmh_scale.h, uploaded once.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "jmh_launch.h"
#include "jmh_scale.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

static float median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static void shape(const char *name, int w, int h, int ow, int oh, int filter, int bd, int reps, hipStream_t st) {
    const int sW = (w + 15) & ~15, sH = (h + 15) & ~15, W = (ow + 15) & ~15, H = (oh + 15) & ~15, es = bd > 8 ? 2 : 1;
    const size_t ssize = (size_t)sW * sH * 3 / 2 * es, dsize = (size_t)W * H * 3 / 2 * es;
    if (jms_check_setting(filter, 0, ow, oh, W, H) || jms_check(w, h, ow, oh, filter)) { fprintf(stderr, "%s: refused\n", name); exit(1); }
    ScaleArgs a;
    std::vector<uint8_t> blob;
    size_t off[2][4];
    for (int pc = 0; pc < 2; pc++) {
        const int ns[2] = {pc ? w / 2 : w, pc ? h / 2 : h}, nd[2] = {pc ? ow / 2 : ow, pc ? oh / 2 : oh};
        int T[2];
        for (int ax = 0; ax < 2; ax++) {
            std::vector<int32_t> first(nd[ax]);
            std::vector<int16_t> taps((size_t)nd[ax] * JMS_TAPS_MAX);
            if (jms_taps(ns[ax], nd[ax], filter, 0, first.data(), taps.data(), &T[ax])) { fprintf(stderr, "%s: no tables\n", name); exit(1); }
            if (ax && jms_span(first.data(), nd[1], T[1], pc ? H / 2 : H) > JMS_SPAN_MAX) { fprintf(stderr, "%s: span\n", name); exit(1); }
            const int np = ax ? JMS_VPAIRS : JMS_HPAIRS;
            off[pc][ax] = blob.size();
            blob.resize(blob.size() + (((size_t)nd[ax] * 4 + 15) & ~(size_t)15));
            memcpy(blob.data() + off[pc][ax], first.data(), (size_t)nd[ax] * 4);
            off[pc][2 + ax] = blob.size();
            blob.resize(blob.size() + (((size_t)nd[ax] * np * 4 + 15) & ~(size_t)15));
            jms_pack_axis(first.data(), taps.data(), nd[ax], T[ax], ax, (uint32_t *)(blob.data() + off[pc][2 + ax]));
        }
        a.nph[pc] = T[0] / 2; a.npv[pc] = T[1] / 2 + 1; a.tv_taps[pc] = T[1];
    }
    uint8_t *src, *dst, *cpy_s, *cpy_d, *tab;
    CK(hipMalloc(&src, ssize)); CK(hipMalloc(&dst, dsize)); CK(hipMalloc(&cpy_s, ssize + dsize)); CK(hipMalloc(&cpy_d, ssize + dsize));
    CK(hipMalloc(&tab, blob.size()));
    CK(hipMemset(src, 1, ssize));
    CK(hipMemset(cpy_s, 1, ssize + dsize));
    CK(hipMemcpy(tab, blob.data(), blob.size(), hipMemcpyHostToDevice));
    a.src = src; a.dst = dst; a.w = w; a.h = h; a.sW = sW; a.sH = sH; a.ow = ow; a.oh = oh; a.W = W; a.H = H;
    for (int pc = 0; pc < 2; pc++) {
        a.fh[pc] = (const int32_t *)(tab + off[pc][0]); a.fv[pc] = (const int32_t *)(tab + off[pc][1]);
        a.th[pc] = (const uint32_t *)(tab + off[pc][2]); a.tv[pc] = (const uint32_t *)(tab + off[pc][3]);
    }
    a.maxv = (1 << bd) - 1; a.P = 14 - bd;
    hipEvent_t e[4];
    for (auto &x : e) CK(hipEventCreate(&x));
    std::vector<float> tk, tc;
    for (int r = 0; r < reps + 10; r++) {
        CK(hipEventRecord(e[0], st));
        CK(jmh_launch_scale(a, st));
        CK(hipEventRecord(e[1], st));
        CK(hipEventRecord(e[2], st));
        CK(hipMemcpyAsync(cpy_d, cpy_s, ssize + dsize, hipMemcpyDeviceToDevice, st));
        CK(hipEventRecord(e[3], st));
        CK(hipStreamSynchronize(st));
        float a_ms, b_ms;
        CK(hipEventElapsedTime(&a_ms, e[0], e[1])); CK(hipEventElapsedTime(&b_ms, e[2], e[3]));
        if (r >= 10) { tk.push_back(a_ms); tc.push_back(b_ms); }   // the first ten warm up
    }
    const float k = median(tk), c = median(tc);
    printf("%-26s %4dx%-4d -> %4dx%-4d %2d bits taps %2d/%2d  %9zu + %8zu bytes  k_scale %7.1f us (min %7.1f)  copy D2D %7.1f us (min %7.1f)  ratio %.2f\n",
           name, w, h, ow, oh, bd, 2 * a.nph[0], a.tv_taps[0], ssize, dsize, 1e3 * k, 1e3 * *std::min_element(tk.begin(), tk.end()), 1e3 * c,
           1e3 * *std::min_element(tc.begin(), tc.end()), k / c);
    for (auto &x : e) CK(hipEventDestroy(x));
    CK(hipFree(src)); CK(hipFree(dst)); CK(hipFree(cpy_s)); CK(hipFree(cpy_d)); CK(hipFree(tab));
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 200;
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    printf("k_scale against hipMemcpyAsync D2D of source + destination bytes, HIP events, alternating, median of %d\n", reps);
    shape("2160p->1080p I420 lanczos3", 3840, 2160, 1920, 1080, JMS_LANCZOS3, 8, reps, st);
    shape("2160p->1080p I420 bilinear", 3840, 2160, 1920, 1080, JMS_BILINEAR, 8, reps, st);
    shape("2160p->1080p I010 lanczos3", 3840, 2160, 1920, 1080, JMS_LANCZOS3, 10, reps, st);
    shape("2160p->1080p I010 bilinear", 3840, 2160, 1920, 1080, JMS_BILINEAR, 10, reps, st);
    shape("1080p->1080p I420 identity", 1920, 1080, 1920, 1080, JMS_LANCZOS3, 8, reps, st);
    shape("1080p->1080p I010 identity", 1920, 1080, 1920, 1080, JMS_LANCZOS3, 10, reps, st);
    CK(hipStreamDestroy(st));
    return 0;
}
