// Part of genie_hip.hip (one translation unit, included inside its anonymous namespace): the optimizer step of a training batch -- the
// ranks' gradient parts summed in rank order and Adam (train_GENIE_model.py:1383, :1861) applied to the flat parameter blob, one launch.

// ------------------------------------------------------------------------------------------------
// g[j] = ((0 + part_0[j]) + part_1[j]) + ...   in part order, fp32, starting from 0.0f -- the bits of `g = zeros; g += part_r` part by
// part, whatever schedule a collective would have used: the sum of a sample-parallel step is made HERE, after an all-gather, so that the
// weights depend on (batch, world) alone. The sum is made with contraction off. Then torch.optim.Adam's single-tensor update with its
// defaults (no weight decay, no amsgrad, not maximize), operation by operation as torch's CPU kernels round it -- the two fused
// multiply-adds are written out (`fmaf`), nothing is left to the compiler's contraction:
//   m = fma(g - m, w1, m)                         `exp_avg.lerp_(grad, 1 - beta1)`, w1 = (float)(1 - beta1) < 0.5
//   v = fma(w2 * g, g, v * beta2)                 `exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)`
//   p = p + (-step_size * m) / (sqrt(v) / bc2_sqrt + eps)        `param.addcdiv_(exp_avg, denom, value=-step_size)`
// step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) are formed by the host in double and rounded to fp32 once, as
// torch passes its Python scalars; v_sqrt_f32 / v_div_f32 sequences are the correctly rounded ones (hipcc's default). An element with
// g = m = v = 0 keeps its bits in all three arrays: m = fma(0, w1, 0), v = fma(0, 0, 0 * beta2), p = p + (-step_size * 0) / eps = p + (-0).
// One thread owns four consecutive floats: 16-byte loads and stores of the state (p, m, v, grad_out) and of the parts where the
// pointers (and, with more than one part, part_stride) allow -- two independent template flags, since a part buffer of n + 1 floats per
// rank leaves only part 0 aligned -- and element by element otherwise and in the last, partial quad. 64-bit offsets; 256 threads span
// 1 024 floats per workgroup up to AD_MAX_WG workgroups, beyond which threads stride. No LDS, no atomics, no verdict word: nothing here
// can fail on the device. grad_out must not overlap the parts.
// ------------------------------------------------------------------------------------------------
constexpr int AD_BLOCK = 256;
constexpr int AD_MAX_WG = 1024;
constexpr int AD_MAX_PARTS = 32;

struct AdScalars {
    float w1, beta2, w2, neg_step_size, bc2_sqrt, eps;
};

template <bool VEC_STATE, bool VEC_PARTS>
__global__ __launch_bounds__(AD_BLOCK) void k_adam_step(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long long n,
                                                         const float* __restrict__ parts, int n_parts, long long part_stride,
                                                         float* __restrict__ gout, AdScalars s) {
#pragma clang fp contract(off)
    const long long n_quad = (n + 3) >> 2;
    const long long stride = (long long)gridDim.x * AD_BLOCK;
    for (long long q = (long long)blockIdx.x * AD_BLOCK + threadIdx.x; q < n_quad; q += stride) {
        const long long j = q << 2;
        const bool full = j + 4 <= n;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < n_parts; ++r) {
            const float* src = parts + (long long)r * part_stride + j;
            float x[4];
            if (VEC_PARTS && full) {
                const float4 t = *(const float4*)src;
                x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = j + k < n ? src[k] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = g[k] + x[k];
        }
        float pv[4], mv[4], vv[4];
        if (VEC_STATE && full) {
            const float4 a = *(const float4*)(p + j), b = *(const float4*)(m + j), c = *(const float4*)(v + j);
            pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
            mv[0] = b.x; mv[1] = b.y; mv[2] = b.z; mv[3] = b.w;
            vv[0] = c.x; vv[1] = c.y; vv[2] = c.z; vv[3] = c.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = j + k < n;
                pv[k] = in ? p[j + k] : 0.f;
                mv[k] = in ? m[j + k] : 0.f;
                vv[k] = in ? v[j + k] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = g[k] - mv[k];
            mv[k] = fmaf(d, s.w1, mv[k]);
            const float vb = vv[k] * s.beta2;
            const float wg = s.w2 * g[k];
            vv[k] = fmaf(wg, g[k], vb);
            const float sq = sqrtf(vv[k]);
            const float sc = sq / s.bc2_sqrt;
            const float den = sc + s.eps;
            const float sm = s.neg_step_size * mv[k];
            const float upd = sm / den;
            pv[k] = pv[k] + upd;
        }
        if (VEC_STATE && full) {
            *(float4*)(p + j) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            *(float4*)(m + j) = make_float4(mv[0], mv[1], mv[2], mv[3]);
            *(float4*)(v + j) = make_float4(vv[0], vv[1], vv[2], vv[3]);
            if (gout) *(float4*)(gout + j) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j + k < n) {
                    p[j + k] = pv[k];
                    m[j + k] = mv[k];
                    v[j + k] = vv[k];
                    if (gout) gout[j + k] = g[k];
                }
        }
    }
}
