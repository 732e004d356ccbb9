/*
 * pgx_mlp.h -- what the policy units (pgx_actor.hip, pgx_actor_critic.hip) share: one Linear over a
 * workgroup's env tile as v_mfma_f32_16x16x4_f32 on activations kept in LDS, and the kernel that
 * packs torch-layout weights for it.  Arithmetic contract and packed layout: include/pgx.h, "Actor".
 * Everything here has internal linkage: each unit compiles its own copy.
 */
#ifndef PGX_MLP_H
#define PGX_MLP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int WAVES = 4;        /* waves of a forward workgroup */
constexpr int NACC = 4;         /* output tiles a wave accumulates side by side */

typedef float f32x4 __attribute__((ext_vector_type(4)));

/* One Linear over the workgroup's MT x 16 envs: lds[in_off..] (row stride S_in) -> lds[out_off..]
 * (row stride S_out) */
template <int MT>
__device__ __forceinline__ void linear_layer(float* lds, int in_off, int out_off, const float* __restrict__ P,
                                             const float* __restrict__ bias, int nkb, int ntiles, int S_in, int S_out,
                                             bool relu, int lane, int wave) {
    const int col = lane & 15, kq = lane >> 4;
    const f32x4* Pv = reinterpret_cast<const f32x4*>(P);
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t0 = wave; t0 < ntiles; t0 += WAVES * NACC) {
        f32x4 acc[NACC][MT], w[NACC];
        bool valid[NACC];
#pragma unroll
        for (int i = 0; i < NACC; i++) {
            const int tile = t0 + WAVES * i;
            valid[i] = tile < ntiles;   /* the same in every lane of the wave */
            const float b = valid[i] ? bias[tile * 16 + col] : 0.0f;
#pragma unroll
            for (int m = 0; m < MT; m++) acc[i][m] = f32x4{b, b, b, b};
            w[i] = valid[i] ? Pv[tile * 64 + lane] : zero4;
        }
        for (int kb = 0; kb < nkb; kb++) {
            f32x4 wn[NACC];
#pragma unroll
            for (int i = 0; i < NACC; i++) {
                const int tile = t0 + WAVES * i;
                wn[i] = (valid[i] && kb + 1 < nkb) ? Pv[((kb + 1) * ntiles + tile) * 64 + lane] : zero4;
            }
#pragma unroll
            for (int s = 0; s < 4; s++) {
                float a[MT];
#pragma unroll
                for (int m = 0; m < MT; m++) a[m] = lds[in_off + (m * 16 + col) * S_in + kb * 16 + 4 * s + kq];
#pragma unroll
                for (int i = 0; i < NACC; i++) {
                    if (!valid[i]) continue;
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        acc[i][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], w[i][s], acc[i][m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < NACC; i++) w[i] = wn[i];
        }
#pragma unroll
        for (int i = 0; i < NACC; i++) {
            if (!valid[i]) continue;
            const int tile = t0 + WAVES * i;
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[i][m][r];
                    if (relu) v = v > 0.0f ? v : 0.0f;
                    lds[out_off + (m * 16 + kq * 4 + r) * S_out + tile * 16 + col] = v;
                }
        }
    }
}

/* the same with one row stride S on both sides */
template <int MT>
__device__ __forceinline__ void linear_layer(float* lds, int in_off, int out_off, const float* __restrict__ P,
                                             const float* __restrict__ bias, int nkb, int ntiles, int S, bool relu,
                                             int lane, int wave) {
    linear_layer<MT>(lds, in_off, out_off, P, bias, nkb, ntiles, S, S, relu, lane, wave);
}

/* plain [out, in] weights and [out] bias into the packed layout, at rows row_off.. of the Linear's
 * output; the padding was zeroed at create and is never written */
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                   float* P, float* bp, int out, int in, int ntiles, int row_off) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < out * in) {
        const int o = idx / in, k = idx - o * in;
        const int row = o + row_off;
        const int tile = row >> 4, j = row & 15, kb = k >> 4, s = (k >> 2) & 3, kq = k & 3;
        P[((size_t)(kb * ntiles + tile) * 64 + kq * 16 + j) * 4 + s] = W[idx];
    } else if (idx < out * in + out) {
        const int o = idx - out * in;
        bp[o + row_off] = b[o];
    }
}

}  // namespace

#endif /* PGX_MLP_H */
