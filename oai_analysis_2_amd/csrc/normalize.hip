// Intensity windowing (the step just before the hot path):
//   image_normalize(image, 0.1, 99.9, 0, 1)   oai_analysis/dask_processing.py:10-26, called at :75 and :177
//     window_min/max = np.percentile(array, q)            (exact order statistics + linear interpolation)
//     itk.IntensityWindowingImageFilter[F,F]              (x<wmin -> omin; x>wmax -> omax; else x*factor+offset in double)
// On the device the two percentiles are found EXACTLY by the 4-pass 8-bit radix select of csrc/radix_select.h
// (4 ranks at once: k_lo, k_lo+1, k_hi, k_hi+1), then one streaming pass applies the window.  HBM-bound: 5 reads + 1 write of the volume.
#include "common.h"
#include "radix_select.h"

namespace {

using namespace oai;

constexpr int kThreads = 256;

struct WindowState {                 // lives in the caller's workspace
    SelectState sel;
    float window[2];                 // interpolated percentiles (wmin, wmax)
};

__global__ void select_init_kernel(WindowState* st, unsigned long long r0, unsigned long long r1, unsigned long long r2, unsigned long long r3) {
    const int t = threadIdx.x;
    if (t < kSelectRanks) { st->sel.prefix[t] = 0; st->sel.rank[t] = t == 0 ? r0 : t == 1 ? r1 : t == 2 ? r2 : r3; }
    select_clear_hist(&st->sel);
}

__global__ void __launch_bounds__(kThreads) select_hist_kernel(const float* __restrict__ x, size_t n, int pass, WindowState* st) {
    select_hist_pass<kThreads>(&st->sel, pass, [&](auto add) {
        for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) add(x[i]);
    });
}

__global__ void select_scan_kernel(int pass, WindowState* st) { select_scan_step(&st->sel, pass); }

__global__ void window_params_kernel(WindowState* st, float g_lo, float g_hi) {
    if (threadIdx.x < 2)
        st->window[threadIdx.x] = numpy_lerp(st->sel.value[2 * threadIdx.x], st->sel.value[2 * threadIdx.x + 1], threadIdx.x == 0 ? g_lo : g_hi);
}

__global__ void __launch_bounds__(kThreads) window_apply_kernel(const float* __restrict__ x, size_t n, const WindowState* st,
                                                                float omin, float omax, float* __restrict__ out) {
    const float wmin = st->window[0], wmax = st->window[1];
    // the functor rounds the product and the sum one after the other; a fused multiply-add gives other bits (x == wmin would not map to
    // out_min exactly), so nothing here may be contracted
    const double factor = ((double)omax - (double)omin) / ((double)wmax - (double)wmin);
    const double offset = __dsub_rn((double)omin, __dmul_rn((double)wmin, factor));
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)gridDim.x * kThreads) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = r[j] < wmin ? omin : (r[j] > wmax ? omax : (float)__dadd_rn(__dmul_rn((double)r[j], factor), offset));
        reinterpret_cast<float4*>(out)[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
        const float v = x[i];
        out[i] = v < wmin ? omin : (v > wmax ? omax : (float)__dadd_rn(__dmul_rn((double)v, factor), offset));
    }
}

}  // namespace

extern "C" {

size_t oai_image_normalize_workspace_bytes(void) { return oai::round256(sizeof(WindowState)); }

int oai_image_normalize(const float* in, size_t n, float pct_lo, float pct_hi, float out_min, float out_max,
                        float* out, float* window_out_dev, void* ws, size_t ws_bytes, void* stream) {
    OAI_CHECK_ARG(in && out && ws, "oai_image_normalize: null pointer");
    OAI_CHECK_ARG(n >= 2, "oai_image_normalize: need at least 2 voxels");
    OAI_CHECK_ARG(pct_lo >= 0.0f && pct_hi <= 100.0f && pct_lo < pct_hi, "oai_image_normalize: percentiles must satisfy 0 <= lo < hi <= 100");
    OAI_CHECK_ARG((reinterpret_cast<uintptr_t>(in) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "oai_image_normalize: buffers must be 16-byte aligned");
    OAI_CHECK_WORKSPACE("oai_image_normalize", ws_bytes, oai_image_normalize_workspace_bytes());
    hipStream_t st = (hipStream_t)stream;
    WindowState* s = reinterpret_cast<WindowState*>(ws);
    unsigned long long k[4];
    float g_lo, g_hi;
    numpy_virtual_index(n, pct_lo, k[0], k[1], g_lo);
    numpy_virtual_index(n, pct_hi, k[2], k[3], g_hi);
    select_init_kernel<<<1, 256, 0, st>>>(s, k[0], k[1], k[2], k[3]);
    OAI_CHECK_LAUNCH();
    size_t blocks = (n + kThreads * 16 - 1) / (kThreads * 16);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    for (int pass = 0; pass < 4; ++pass) {
        select_hist_kernel<<<(unsigned)blocks, kThreads, 0, st>>>(in, n, pass, s);
        OAI_CHECK_LAUNCH();
        select_scan_kernel<<<1, 256, 0, st>>>(pass, s);
        OAI_CHECK_LAUNCH();
    }
    window_params_kernel<<<1, 64, 0, st>>>(s, g_lo, g_hi);
    OAI_CHECK_LAUNCH();
    window_apply_kernel<<<(unsigned)blocks, kThreads, 0, st>>>(in, n, s, out_min, out_max, out);
    OAI_CHECK_LAUNCH();
    if (window_out_dev) OAI_CHECK_HIP(hipMemcpyAsync(window_out_dev, s->window, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return OAI_OK;
}

}  // extern "C"
