// Adam over a list of fp32 tensors in ONE launch (round 3).  The reference's drivers build torch.optim.Adam (train_tile.py:282,
// train_image.py:476, train_seg.py:309); torch's fused implementation of that update is 5 multi_tensor_apply launches at 2.9 TB/s
// on the ResNet-50 tile step (658 MB of parameter / gradient / moment traffic, 0.23 ms of a 7.4 ms step).  Here: a device table of
// (p, m, v, n), the gradients' addresses BY VALUE in the kernel arguments (they change every step: autograd hands out fresh
// tensors), a device list of 16 Ki-element chunks, one workgroup per chunk, 16 bytes per lane.
//   g' = g + weight_decay * p            (torch.optim.Adam's L2 form, not AdamW)
//   m  = m + (1 - beta1) * (g' - m)      (lerp, as torch)
//   v  = beta2 * v + (1 - beta2) * g'^2
//   p  = p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// SGD with momentum (second half of the file): what the drivers train with whenever a scheduler is given (train_tile.py:280-303,
// train_seg.py:289-312, train_image.py:483-508: optim.SGD(lr, momentum=0.9, weight_decay=1e-4)), on the same tables and chunk list.
#include "cs_common.h"
#include <math.h>

namespace {

constexpr int kAdamChunk = 16384;
constexpr int kAdamMaxTensors = 320;

struct AdamGrads { const float* g[kAdamMaxTensors]; };

// (omb1 = 1 - beta1 and omb2 = 1 - beta2 arrive rounded from DOUBLE, as torch forms them: 1.f - 0.999f is off by 1.3e-5 relative)
__device__ __forceinline__ void adam1(float& p, float& m, float& v, float g, float step_size, float inv_sqrt_bc2, float omb1, float beta2,
                                      float omb2, float eps, float wd) {
    g = g + wd * p;
    m = m + omb1 * (g - m);
    v = beta2 * v + omb2 * g * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
    p = p - step_size * (m / denom);
}

// `coef` (capturable form, cs_adam_step_dev): the per-tensor (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) pairs adam_prep_kernel left in
// device memory for this launch; NULL: the two by-value arguments.
__global__ __launch_bounds__(256) void adam_multi_kernel(const CsAdamTensor* __restrict__ tensors, AdamGrads grads, const int2* __restrict__ chunks,
                                                         int t0, float step_size, float inv_sqrt_bc2, float omb1, float beta2, float omb2, float eps, float wd,
                                                         const float2* __restrict__ coef) {
    const int2 ch = chunks[blockIdx.x];                      // (tensor index, first element / kAdamChunk)
    const CsAdamTensor t = tensors[ch.x];
    if (coef) {
        const float2 c2 = coef[ch.x];
        step_size = c2.x;
        inv_sqrt_bc2 = c2.y;
    }
    const float* __restrict__ g = nullptr;
    {
        const int li = ch.x - t0;
        // (static indexing of a by-value table: a runtime index would copy the whole table to scratch)
        const float* const* gt = grads.g;
        g = gt[li];
    }
    const long long begin = (long long)ch.y * kAdamChunk;
    long long end = begin + kAdamChunk;
    if (end > t.n) end = t.n;
    float* __restrict__ p = t.p;
    float* __restrict__ m = t.m;
    float* __restrict__ v = t.v;
    const bool vec = ((((unsigned long long)p) | ((unsigned long long)m) | ((unsigned long long)v) | ((unsigned long long)g)) & 15ull) == 0ull;
    if (vec) {
        const long long end4 = begin + ((end - begin) & ~3ll);
        for (long long i = begin + 4ll * threadIdx.x; i < end4; i += 1024) {
            float4 pp = *reinterpret_cast<const float4*>(p + i), mm = *reinterpret_cast<const float4*>(m + i);
            float4 vv = *reinterpret_cast<const float4*>(v + i);
            const float4 gg = *reinterpret_cast<const float4*>(g + i);
            adam1(pp.x, mm.x, vv.x, gg.x, step_size, inv_sqrt_bc2, omb1, beta2, omb2, eps, wd);
            adam1(pp.y, mm.y, vv.y, gg.y, step_size, inv_sqrt_bc2, omb1, beta2, omb2, eps, wd);
            adam1(pp.z, mm.z, vv.z, gg.z, step_size, inv_sqrt_bc2, omb1, beta2, omb2, eps, wd);
            adam1(pp.w, mm.w, vv.w, gg.w, step_size, inv_sqrt_bc2, omb1, beta2, omb2, eps, wd);
            *reinterpret_cast<float4*>(p + i) = pp;
            *reinterpret_cast<float4*>(m + i) = mm;
            *reinterpret_cast<float4*>(v + i) = vv;
        }
        for (long long i = end4 + threadIdx.x; i < end; i += 256) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam1(pp, mm, vv, g[i], step_size, inv_sqrt_bc2, omb1, beta2, omb2, eps, wd);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    } else {
        for (long long i = begin + threadIdx.x; i < end; i += 256) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam1(pp, mm, vv, g[i], step_size, inv_sqrt_bc2, omb1, beta2, omb2, eps, wd);
            p[i] = pp; m[i] = mm; v[i] = vv;
        }
    }
}

// Capturable form: the step counts live in DEVICE memory (one fp32 scalar per tensor: torch.optim.Adam(capturable=True)'s state
// layout), so a launch captured into a HIP graph advances them at every replay.  One thread per tensor: t = ++step, the bias
// corrections in double (device pow), the learning rate from a device double when the caller keeps one (schedulers change it
// between replays of a captured step).
__global__ void adam_prep_kernel(float* const* __restrict__ steps, int t0, int n, const double* __restrict__ lr_dev, double lr, double beta1,
                                 double beta2, float2* __restrict__ coef) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* sp = steps[t0 + i];
    const float t = *sp + 1.0f;
    *sp = t;
    const double l = lr_dev ? *lr_dev : lr;
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    coef[t0 + i] = make_float2((float)(l / bc1), (float)(1.0 / sqrt(bc2)));
}

// ---- host side.  What every entry point takes: device tables, a HOST array of gradient pointers, 1..320 tensors, a chunk list
bool common_args_ok(const void* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks) {
    return tensors_dev && grads_host && chunks_dev && t0 >= 0 && n_tensors >= 1 && n_tensors <= kAdamMaxTensors && n_chunks >= 1;
}

// the gradients' addresses into the by-value kernel argument; false at a NULL among them: nothing may be launched then
bool pack_grads(const void* const* grads_host, int n_tensors, AdamGrads* gr) {
    for (int i = 0; i < n_tensors; ++i)
        if (!(gr->g[i] = reinterpret_cast<const float*>(grads_host[i]))) return false;
    return true;
}

// `steps_dev` (capturable form): adam_prep_kernel leaves the coefficients in `coef` first; NULL: the two by-value coefficients
int adam_launch(const char* who, const CsAdamTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks,
                float* const* steps_dev, float2* coef, const double* lr_dev, double lr, float step_size, float inv_sqrt_bc2, double beta1, double beta2,
                double eps, double weight_decay, void* stream) {
    AdamGrads gr{};
    CS_CHECK_ARG(pack_grads(grads_host, n_tensors, &gr), who);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (steps_dev) {
        hipLaunchKernelGGL(adam_prep_kernel, dim3((unsigned)((n_tensors + 63) / 64)), dim3(64), 0, st, steps_dev, t0, n_tensors, lr_dev, lr, beta1, beta2, coef);
        CS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, tensors_dev, gr, reinterpret_cast<const int2*>(chunks_dev), t0,
                       step_size, inv_sqrt_bc2, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay, coef);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

}  // namespace

extern "C" int cs_adam_chunk_elems(void) { return kAdamChunk; }
extern "C" int cs_adam_max_tensors(void) { return kAdamMaxTensors; }

extern "C" int cs_adam_step(const CsAdamTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev,
                            int n_chunks, double lr, double beta1, double beta2, double eps, double weight_decay, double step, void* stream) {
    CS_CHECK_ARG(common_args_ok(tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks),
                 "adam_step: 1..320 tensors per call, device tables, a HOST array of gradient pointers");
    CS_CHECK_ARG(step >= 1.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_step: step >= 1, betas in [0, 1)");
    // scalar arithmetic in double, like torch's fused kernel: only the results are rounded to fp32
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    return adam_launch("adam_step: NULL gradient", tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks, nullptr, nullptr, nullptr, lr,
                       (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), beta1, beta2, eps, weight_decay, stream);
}

extern "C" int cs_adam_step_dev(const CsAdamTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev,
                                int n_chunks, float* const* steps_dev, float* coef_dev, const double* lr_dev, double lr, double beta1, double beta2,
                                double eps, double weight_decay, void* stream) {
    CS_CHECK_ARG(common_args_ok(tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks) && steps_dev && coef_dev,
                 "adam_step_dev: 1..320 tensors per call, device tables (tensors, chunks, step pointers, coefficient scratch), a HOST array of gradient pointers");
    CS_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_step_dev: betas in [0, 1)");
    return adam_launch("adam_step_dev: NULL gradient", tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks, steps_dev,
                       reinterpret_cast<float2*>(coef_dev), lr_dev, lr, 0.0f, 0.0f, beta1, beta2, eps, weight_decay, stream);
}

// ---- SGD (torch.optim.SGD, single-tensor form) -------------------------------------------------------------------------------
//   g' = g + weight_decay * p
//   momentum != 0:  first step of the tensor: buf = g'       later: buf = momentum * buf + (1 - dampening) * g'
//                   nesterov: g' = g' + momentum * buf       otherwise: g' = buf
//   p  = p - lr * g'
// 20 B per parameter (read p, g, buf; write p, buf); 16 B on a tensor's first step (buf is only written), 12 B without momentum.
namespace {

enum { kSgdPlain = 0, kSgdFirst = 1, kSgdLater = 2 };      // no buffer / buf = g' / buf = momentum * buf + omd * g'

template <int kMode>
__device__ __forceinline__ void sgd1(float& p, float& b, float g, float lr, float mom, float omd, float wd, bool nesterov) {
    g = g + wd * p;
    if (kMode != kSgdPlain) {
        b = kMode == kSgdFirst ? g : mom * b + omd * g;
        g = nesterov ? g + mom * b : b;
    }
    p = p - lr * g;
}

// one chunk [begin, end) of one tensor; `buf` is neither read nor written in kSgdPlain and only written in kSgdFirst
template <int kMode>
__device__ __forceinline__ void sgd_chunk(float* __restrict__ p, float* __restrict__ buf, const float* __restrict__ g, long long begin, long long end,
                                          float lr, float mom, float omd, float wd, bool nesterov) {
    unsigned long long bits = ((unsigned long long)p) | ((unsigned long long)g);
    if (kMode != kSgdPlain) bits |= (unsigned long long)buf;
    const long long end4 = (bits & 15ull) == 0ull ? begin + ((end - begin) & ~3ll) : begin;      // unaligned: the scalar loop takes everything
    for (long long i = begin + 4ll * threadIdx.x; i < end4; i += 1024) {
        float4 pp = *reinterpret_cast<const float4*>(p + i), bb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kMode == kSgdLater) bb = *reinterpret_cast<const float4*>(buf + i);
        const float4 gg = *reinterpret_cast<const float4*>(g + i);
        sgd1<kMode>(pp.x, bb.x, gg.x, lr, mom, omd, wd, nesterov);
        sgd1<kMode>(pp.y, bb.y, gg.y, lr, mom, omd, wd, nesterov);
        sgd1<kMode>(pp.z, bb.z, gg.z, lr, mom, omd, wd, nesterov);
        sgd1<kMode>(pp.w, bb.w, gg.w, lr, mom, omd, wd, nesterov);
        *reinterpret_cast<float4*>(p + i) = pp;
        if (kMode != kSgdPlain) *reinterpret_cast<float4*>(buf + i) = bb;
    }
    for (long long i = end4 + threadIdx.x; i < end; i += 256) {
        float pp = p[i], bb = 0.f;
        if (kMode == kSgdLater) bb = buf[i];
        sgd1<kMode>(pp, bb, g[i], lr, mom, omd, wd, nesterov);
        p[i] = pp;
        if (kMode != kSgdPlain) buf[i] = bb;
    }
}

// `hyper` (capturable form, cs_sgd_step_dev): (lr, momentum) as two doubles in device memory, rounded to fp32 here as the host form
// rounds its arguments; NULL: the two by-value arguments.  A tensor without a buffer takes the plain update whatever the momentum.
__global__ __launch_bounds__(256) void sgd_multi_kernel(const CsSgdTensor* __restrict__ tensors, AdamGrads grads, const int2* __restrict__ chunks, int t0,
                                                        float lr, float mom, float omd, float wd, int nesterov, int first,
                                                        const double* __restrict__ hyper) {
    const int2 ch = chunks[blockIdx.x];                      // (tensor index, first element / kAdamChunk)
    const CsSgdTensor t = tensors[ch.x];
    if (hyper) {
        lr = (float)hyper[0];
        mom = (float)hyper[1];
    }
    const float* const* gt = grads.g;
    const float* __restrict__ g = gt[ch.x - t0];
    const long long begin = (long long)ch.y * kAdamChunk;
    long long end = begin + kAdamChunk;
    if (end > t.n) end = t.n;
    if (t.buf == nullptr) sgd_chunk<kSgdPlain>(t.p, nullptr, g, begin, end, lr, mom, omd, wd, false);
    else if (first) sgd_chunk<kSgdFirst>(t.p, t.buf, g, begin, end, lr, mom, omd, wd, nesterov != 0);
    else sgd_chunk<kSgdLater>(t.p, t.buf, g, begin, end, lr, mom, omd, wd, nesterov != 0);
}

int sgd_launch(const char* who, const CsSgdTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks,
               double lr, double momentum, double dampening, double weight_decay, int nesterov, int first, const double* hyper_dev, void* stream) {
    AdamGrads gr{};
    CS_CHECK_ARG(pack_grads(grads_host, n_tensors, &gr), who);
    // the scalars as torch forms them: python doubles, 1 - dampening in double, each rounded to fp32 once
    hipLaunchKernelGGL(sgd_multi_kernel, dim3((unsigned)n_chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), tensors_dev, gr,
                       reinterpret_cast<const int2*>(chunks_dev), t0, (float)lr, (float)momentum, (float)(1.0 - dampening), (float)weight_decay, nesterov,
                       first, hyper_dev);
    CS_LAUNCH_CHECK();
    return CS_OK;
}

}  // namespace

extern "C" int cs_sgd_step(const CsSgdTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks,
                           double lr, double momentum, double dampening, double weight_decay, int nesterov, int first, void* stream) {
    CS_CHECK_ARG(common_args_ok(tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks),
                 "sgd_step: 1..320 tensors per call, device tables, a HOST array of gradient pointers");
    CS_CHECK_ARG(lr >= 0.0 && momentum >= 0.0 && weight_decay >= 0.0, "sgd_step: lr, momentum and weight_decay >= 0");
    CS_CHECK_ARG(!nesterov || (momentum > 0.0 && dampening == 0.0), "sgd_step: nesterov requires momentum > 0 and dampening == 0");
    return sgd_launch("sgd_step: NULL gradient", tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks, lr, momentum, dampening, weight_decay,
                      nesterov, first, nullptr, stream);
}

extern "C" int cs_sgd_step_dev(const CsSgdTensor* tensors_dev, const void* const* grads_host, int t0, int n_tensors, const int* chunks_dev, int n_chunks,
                               const double* hyper_dev, double dampening, double weight_decay, int nesterov, int first, void* stream) {
    CS_CHECK_ARG(common_args_ok(tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks) && hyper_dev,
                 "sgd_step_dev: 1..320 tensors per call, device tables (tensors, chunks, the (lr, momentum) doubles), a HOST array of gradient "
                 "pointers");
    CS_CHECK_ARG(weight_decay >= 0.0, "sgd_step_dev: weight_decay >= 0");
    // (momentum > 0 cannot be checked here: it lives on the device; a tensor without a buffer takes the plain update)
    CS_CHECK_ARG(!nesterov || dampening == 0.0, "sgd_step_dev: nesterov requires dampening == 0");
    return sgd_launch("sgd_step_dev: NULL gradient", tensors_dev, grads_host, t0, n_tensors, chunks_dev, n_chunks, 0.0, 0.0, dampening, weight_decay,
                      nesterov, first, hyper_dev, stream);
}
