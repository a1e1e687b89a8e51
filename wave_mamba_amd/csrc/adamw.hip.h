// adamw.hip.h - the optimizer's device side, for gfx950: AdamW (torch's, amsgrad = False, maximize = False) over a device table of
// addresses, with the exponential moving average of the weights folded into the same pass.  fp32, elementwise: no atomics, no
// memset, bit-identical run to run.
//   adamw_step_kernel    one workgroup per table row {param, grad, exp_avg, exp_avg_sq, ema or 0, count}
//   adamw_count_kernel   one lane: step += 1 unless found_inf is set
// Everything that changes from step to step is read from device memory (lr, step, found_inf, grad_scale), so a launch captured into
// a HIP graph follows a scheduler and the guard; beta1, beta2, eps, weight decay and the EMA decay are launch scalars (doubles).
// Reference: torch.optim.AdamW's single-tensor form, operation for operation (cpu_twin.adamw_step states it in tensor operations):
//   p *= 1 - lr wd;  m = lerp(m, g, 1 - beta1);  v = v beta2 + ((1 - beta2) g) g;  p += (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps)
// and the reference's model_ema (base_model.py:85-92): ema = ema d + (1 - d) p, on the new p.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wm {

constexpr int kAdamwRowWords = 6;            // int64 words per table row (ops.ADAMW_ROW_WORDS)

struct AdamwHyper { double beta1, beta2, eps, weight_decay, ema_decay; };

// The step's scalars, each rounded to fp32 once - exactly the Python floats torch's single-tensor AdamW hands its tensor operations.
struct AdamwScalars { float decay, w1, beta2, omb2, neg_step_size, bc2_sqrt, eps, d, omd, grad_scale; bool scaled; };

// beta^t for an integer-valued t >= 1 by repeated squaring, in double (a float32 counter holds integers up to 2^24 exactly).
__device__ __forceinline__ double adamw_powi(double beta, unsigned t) {
    double r = 1.0, b = beta;
    while (t) {
        if (t & 1u) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__device__ __forceinline__ AdamwScalars adamw_scalars(const AdamwHyper h, float lr, float step, const float* grad_scale) {
    const double lr_d = (double)lr;
    const unsigned t = (unsigned)step + 1u;
    const double bc1 = 1.0 - adamw_powi(h.beta1, t);
    const double bc2 = 1.0 - adamw_powi(h.beta2, t);
    AdamwScalars s;
    s.decay = (float)(1.0 - lr_d * h.weight_decay);
    s.w1 = (float)(1.0 - h.beta1);
    s.beta2 = (float)h.beta2;
    s.omb2 = (float)(1.0 - h.beta2);
    s.neg_step_size = (float)(-(lr_d / bc1));
    s.bc2_sqrt = (float)sqrt(bc2);
    s.eps = (float)h.eps;
    s.d = (float)h.ema_decay;
    s.omd = (float)(1.0 - h.ema_decay);
    s.grad_scale = grad_scale ? grad_scale[0] : 1.0f;
    s.scaled = grad_scale != nullptr;
    return s;
}

// One element.  Every operation is rounded on its own, as the tensor operations of the reference round theirs; the one fused
// multiply-add is lerp's, which ATen's vectorised lerp takes as well.
template <bool EMA>
__device__ __forceinline__ void adamw_element(const AdamwScalars& s, float& p, float g, float& m, float& v, float& e) {
#pragma clang fp contract(off)
    if (s.scaled) g = g / s.grad_scale;                                  // torch's fused kernel: grad /= grad_scale (not stored here)
    p = p * s.decay;
    const float diff = g - m;
    m = s.w1 < 0.5f ? __builtin_fmaf(s.w1, diff, m) : __builtin_fmaf(s.w1 - 1.0f, diff, g);
    v = v * s.beta2;
    v = v + (s.omb2 * g) * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + (s.neg_step_size * m) / denom;
    if (EMA) {
        e = e * s.d;
        e = e + s.omd * p;
    }
}

template <bool EMA>
__device__ __forceinline__ void adamw_row_scalar(const AdamwScalars& s, float* p, const float* g, float* m, float* v, float* e,
                                                 long long from, long long n, int first, int stride) {
    for (long long i = from + first; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? e[i] : 0.0f;
        adamw_element<EMA>(s, pi, g[i], mi, vi, ei);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (EMA) e[i] = ei;
    }
}

template <bool EMA>
__device__ __forceinline__ void adamw_row(const AdamwScalars& s, float* p, const float* g, float* m, float* v, float* e, long long n,
                                          bool aligned) {
    const int tid = (int)threadIdx.x;
    if (!aligned) {                                                         // any address off a 16-byte boundary: element by element
        adamw_row_scalar<EMA>(s, p, g, m, v, e, 0, n, tid, 256);
        return;
    }
    const long long n4 = n >> 2;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    float4* e4 = reinterpret_cast<float4*>(e);
    for (long long i = tid; i < n4; i += 256) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        float4 ee = EMA ? e4[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        adamw_element<EMA>(s, pp.x, gg.x, mm.x, vv.x, ee.x);
        adamw_element<EMA>(s, pp.y, gg.y, mm.y, vv.y, ee.y);
        adamw_element<EMA>(s, pp.z, gg.z, mm.z, vv.z, ee.z);
        adamw_element<EMA>(s, pp.w, gg.w, mm.w, vv.w, ee.w);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
        if (EMA) e4[i] = ee;
    }
    adamw_row_scalar<EMA>(s, p, g, m, v, e, 4 * n4, n, tid, 256);           // the last n % 4 floats
}

// table[6 r ..] = {param, grad, exp_avg, exp_avg_sq, ema (0: this row keeps no average), count}.  A row whose addresses (the ema's
// when it has one) all lie on 16-byte boundaries runs on 16-byte accesses with a scalar tail, any other row element by element.
// found_inf (may be NULL) != 0: nothing is written.  grid (n_rows), block (256)
__global__ __launch_bounds__(256) void adamw_step_kernel(const long long* __restrict__ table, const float* __restrict__ lr,
                                                         const float* __restrict__ step, AdamwHyper hyper,
                                                         const float* __restrict__ found_inf, const float* __restrict__ grad_scale) {
    if (found_inf && found_inf[0] != 0.0f) return;
    const long long* row = table + (long long)kAdamwRowWords * blockIdx.x;
    const unsigned long long ap = (unsigned long long)row[0], ag = (unsigned long long)row[1], am = (unsigned long long)row[2],
                             av = (unsigned long long)row[3], ae = (unsigned long long)row[4];
    const long long n = row[5];
    if (n <= 0) return;
    const AdamwScalars s = adamw_scalars(hyper, lr[0], step[0], grad_scale);
    const bool aligned = ((ap | ag | am | av | ae) & 15ull) == 0ull;
    float* p = reinterpret_cast<float*>(ap);
    const float* g = reinterpret_cast<const float*>(ag);
    float* m = reinterpret_cast<float*>(am);
    float* v = reinterpret_cast<float*>(av);
    float* e = reinterpret_cast<float*>(ae);
    if (ae) adamw_row<true>(s, p, g, m, v, e, n, aligned);
    else adamw_row<false>(s, p, g, m, v, e, n, aligned);
}

// The counter's increment: a launch of its own AFTER the update (every workgroup of the update read the old value).  One vector
// lane's plain read-modify-write.  grid (1), block (64)
__global__ __launch_bounds__(64) void adamw_count_kernel(float* __restrict__ step, const float* __restrict__ found_inf) {
    if (threadIdx.x != 0) return;
    if (found_inf && found_inf[0] != 0.0f) return;
    step[0] = step[0] + 1.0f;
}

}  // namespace wm
