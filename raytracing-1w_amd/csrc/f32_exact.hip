/* f32_exact.hip -- DIAGNOSTICS (librt1w_lab.so), not product: the f32 render kernels with 64-bit elementary functions.
 *
 * The same text as context_f32.hip's kernels (rt_f32_kernels.h: the ten __global__ instantiations), compiled with the same options
 * and ONE more macro, RT_F32_ELEMENTARY_F64: sin, cos, atan2, acos and ln of a float are then evaluated by the 64-bit functions of
 * include/rt1w_num.h and rounded once -- what the host build of the f32 core does (oracle/oracle_flat_f32.cpp).  Everything else in
 * the f32 core is + - * /, sqrtf, comparisons and conversions under -ffp-contract=off, so a frame of these kernels must equal the
 * frame of that host build bit for bit (tests/test_f32_twin.py).  The product's kernels differ from these in those five functions
 * only, which rt1w_lab_f32_elementary measures on their own.
 *
 * The kernels reach the product's own plan, launch, resolve and statistics: when the library is loaded it registers exact_kernel_of
 * with librt1w.so (rt1w_internal.h: rt1w_internal_register_f32_kernels), which answers nullptr -- the product's kernel runs -- until
 * rt1w_lab_f32_exact(1) switches it on.  No public flag, no entry of include/rt1w.h, no kernel-choice row: not a product mode.
 *
 * Also here, as the library's other per-element probe: the device half of rt1w_lab_denoise_elementary (rt_denoise.h's falloff and
 * integer power, which the macro above does not touch). */
#define RT_F32_NS rtf32x
#include "rt_f32_kernels.h"

#include "rt1w_internal.h"
#include "rt_denoise.h"
#include "walk_lab.h"

#if !defined(RT_F32_ELEMENTARY_F64)
#error "f32_exact.hip is built with -DRT_F32_ELEMENTARY_F64"
#endif

/* the draw layer of this build's rt1w_num.h on given words (rt_f32_draws.h), for the host and for the device */
namespace rtf32x {
#define double float
#include "rt_f32_draws.h"
#undef double
} // namespace rtf32x

namespace {

bool g_exact_on = false;

const void* exact_kernel_of(int variant, int mode) {
    if (!g_exact_on || variant < 0 || variant >= RT_N_VARIANTS) return nullptr;
    if (mode == 2) return variant == 5 ? reinterpret_cast<const void*>(rtf32x::rt_render_kernel_pw_ss_f32) : nullptr;
    return reinterpret_cast<const void*>(mode ? rtf32x::g_sorted[variant] : rtf32x::g_plain[variant]);
}

struct Registrar { Registrar() { rt1w_internal_register_f32_kernels(exact_kernel_of); } };
static Registrar g_registrar; /* runs when librt1w_lab.so is loaded */

/* the single-precision functions the PRODUCT's f32 kernels call (include/rt1w_num.h, device f32 build), one argument pair per lane */
__global__ void f32_elementary_kernel(int fn, const float* __restrict__ x, const float* __restrict__ y, unsigned long long n, float* __restrict__ out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
        const float a = x[i], b = y[i];
        float r;
        switch (fn) {
            case 0: r = ::sinf(a); break;
            case 1: r = ::cosf(a); break;
            case 2: r = ::atan2f(a, b); break;
            case 3: r = ::acosf(a); break;
            default: r = ::logf(a); break;
        }
        out[i] = r;
    }
}

/* the f32 build's word -> number conversions (include/rt1w_num.h under RT_F32), one word per lane */
__global__ void f32_draws_kernel(int fn, const unsigned long long* __restrict__ words, float lo, float hi, unsigned long long n, float* __restrict__ out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
        out[i] = rtf32x::rt_f32_draw(fn, words[i], lo, hi);
}

/* the two functions the filter kernels build their weights from (rt_denoise.h), one argument per lane: what the device makes of the
 * text that denoise_host.cpp compiles for the host */
__global__ void denoise_elementary_kernel(int fn, const double* __restrict__ x, const uint32_t* __restrict__ e, unsigned long long n, double* __restrict__ out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
        out[i] = fn == 0 ? rt_dn_falloff(x[i]) : rt_dn_powi(x[i], e[i]);
}

} // namespace

/* the device half of rt1w_lab_denoise_elementary (denoise_host.cpp checks the arguments and has the host half); e is read for fn 1 only */
int rt_lab_denoise_elementary_device(int fn, const double* x, const uint32_t* e, uint64_t n, double* out) {
    double *dx = nullptr, *dout = nullptr;
    uint32_t* de = nullptr;
    const size_t bytes = (size_t)n * sizeof(double), ebytes = (size_t)n * sizeof(uint32_t);
    bool ok = hipSetDevice(0) == hipSuccess && hipMalloc((void**)&dx, bytes) == hipSuccess && hipMalloc((void**)&dout, bytes) == hipSuccess &&
              hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && fn == 1) ok = hipMalloc((void**)&de, ebytes) == hipSuccess && hipMemcpy(de, e, ebytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        const unsigned int block = 256;
        const unsigned long long want = (n + block - 1u) / block;
        hipLaunchKernelGGL(denoise_elementary_kernel, dim3((unsigned int)(want < 4096ull ? want : 4096ull)), dim3(block), 0, 0, fn, dx, de, (unsigned long long)n, dout);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (dx) (void)hipFree(dx);
    if (de) (void)hipFree(de);
    if (dout) (void)hipFree(dout);
    if (!ok) { rt1w_internal_set_error("rt1w_lab_denoise_elementary: device error"); return RT1W_ERR_DEVICE; }
    return RT1W_OK;
}

extern "C" int rt1w_lab_f32_exact(int on) {
    const int was = g_exact_on ? 1 : 0;
    g_exact_on = on != 0;
    return was;
}

extern "C" int rt1w_lab_f32_elementary(int device, int fn, const float* x, const float* y, uint64_t n, float* out) {
    if (fn < 0 || fn > 4 || !x || !y || !out || n == 0u) { rt1w_internal_set_error("rt1w_lab_f32_elementary: bad argument"); return RT1W_ERR_INVALID; }
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    bool ok = hipSetDevice(device) == hipSuccess && hipMalloc((void**)&dx, bytes) == hipSuccess && hipMalloc((void**)&dy, bytes) == hipSuccess &&
              hipMalloc((void**)&dout, bytes) == hipSuccess && hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        const unsigned int block = 256;
        const unsigned long long want = (n + block - 1u) / block;
        hipLaunchKernelGGL(f32_elementary_kernel, dim3((unsigned int)(want < 4096ull ? want : 4096ull)), dim3(block), 0, 0, fn, dx, dy, (unsigned long long)n, dout);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (dx) (void)hipFree(dx);
    if (dy) (void)hipFree(dy);
    if (dout) (void)hipFree(dout);
    if (!ok) { rt1w_internal_set_error("rt1w_lab_f32_elementary: device error"); return RT1W_ERR_DEVICE; }
    return RT1W_OK;
}

/* device 0: this translation unit's host pass over the same text; device 1: one lane per word on GPU 0.  The range selectors loop until
 * a draw is below `hi`, so bounds that no draw can satisfy are refused here, before anything runs */
extern "C" int rt1w_lab_f32_draws(int device, int fn, const uint64_t* words, float lo, float hi, uint64_t n, float* out) {
    const bool ranged = fn == 1 || fn == 2 || fn == 5;
    if ((device != 0 && device != 1) || fn < 0 || fn >= RT_F32_DRAW_FNS || !words || !out || n == 0u ||
        (ranged && !(lo < hi && hi - lo < __builtin_huge_valf() && lo > -__builtin_huge_valf()))) {
        rt1w_internal_set_error("rt1w_lab_f32_draws: bad argument");
        return RT1W_ERR_INVALID;
    }
    if (device == 0) {
        for (uint64_t i = 0; i < n; ++i) out[i] = rtf32x::rt_f32_draw(fn, words[i], lo, hi);
        return RT1W_OK;
    }
    unsigned long long* dw = nullptr;
    float* dout = nullptr;
    const size_t wbytes = (size_t)n * sizeof(uint64_t), obytes = (size_t)n * sizeof(float);
    bool ok = hipSetDevice(0) == hipSuccess && hipMalloc((void**)&dw, wbytes) == hipSuccess && hipMalloc((void**)&dout, obytes) == hipSuccess &&
              hipMemcpy(dw, words, wbytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        const unsigned int block = 256;
        const unsigned long long want = (n + block - 1u) / block;
        hipLaunchKernelGGL(f32_draws_kernel, dim3((unsigned int)(want < 4096ull ? want : 4096ull)), dim3(block), 0, 0, fn, dw, lo, hi, (unsigned long long)n, dout);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, dout, obytes, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (dw) (void)hipFree(dw);
    if (dout) (void)hipFree(dout);
    if (!ok) { rt1w_internal_set_error("rt1w_lab_f32_draws: device error"); return RT1W_ERR_DEVICE; }
    return RT1W_OK;
}
