/*
 * pgx_mlp.h -- the device side the policy units (pgx_actor.hip, pgx_actor_critic.hip, pgx_sde_actor.hip,
 * pgx_quantile_critic.hip) share: the plan of one stack of Linears, the feature staging their kernels open with
 * (stage_features dense per env; stage_rows through row strides for every batch launch, with or without action
 * columns), the ordered sums of a batch row's log-probability, one
 * Linear over a workgroup's env tile as v_mfma_f32_16x16x4_f32 on activations kept in LDS, the loop that
 * runs a stack through two LDS regions, the Gaussian draw from the Philox stream, the advance of a
 * device-resident noise word, and the kernel that packs torch-layout weights for the Linear.  Arithmetic
 * contract and packed layout: include/pgx.h, "Actor".  The host side of the same units: pgx_policy.h.
 * Everything here has internal linkage: each unit compiles its own copy.
 */
#ifndef PGX_MLP_H
#define PGX_MLP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pgx.h"
#include "pgx_common.h"   /* philox; leaves fp contract(on) behind, the state everything below compiles under */

namespace {

constexpr int WAVES = 4;        /* waves of a forward workgroup */
constexpr int NACC = 4;         /* output tiles a wave accumulates side by side */
constexpr int THREADS = 64 * WAVES;
constexpr int MAX_LINEAR = PGX_ACTOR_MAX_LAYERS + 1;   /* the hidden layers and the head tile */

typedef float f32x4 __attribute__((ext_vector_type(4)));

/* one stack of Linears: the hidden layers, then a head of one tile (two for 17..32 quantiles) */
struct MlpPlan {
    int32_t n_linear;
    int32_t nkb[MAX_LINEAR], ntiles[MAX_LINEAR];   /* 16-wide k blocks and output tiles per Linear */
    int32_t woff[MAX_LINEAR], boff[MAX_LINEAR];    /* packed weights / padded bias, floats into params */
};

/* features of the workgroup's MT x 16 envs into lds (row stride S), K0 columns each:
 * achieved_goal | desired_goal | observation, +0 past in_dim and past env N */
template <int MT>
__device__ __forceinline__ void stage_features(float* lds, const float* obs, const float* achieved_goal,
                                               const float* desired_goal, int env0, int N, int od, int K0, int S,
                                               int tid) {
    const int in_dim = od + 6;
    for (int idx = tid; idx < MT * 16 * K0; idx += THREADS) {
        const int r = idx / K0, k = idx - r * K0;
        const int e = env0 + r;
        float v = 0.0f;
        if (e < N && k < in_dim) {
            if (k < 3) v = achieved_goal[(size_t)e * 3 + k];
            else if (k < 6) v = desired_goal[(size_t)e * 3 + (k - 3)];
            else v = obs[(size_t)e * od + (k - 6)];
        }
        lds[r * S + k] = v;
    }
}

/* the same for the rows of a batch, each field read through its own row stride (floats), so a HER batch's
 * rows are read where they lie: achieved_goal | desired_goal | observation | action (ad columns; 0 and NULL:
 * none), +0 past od + 6 + ad and past row B */
template <int MT>
__device__ __forceinline__ void stage_rows(float* lds, const float* obs, const float* achieved_goal,
                                           const float* desired_goal, const float* action, int s_obs, int s_ag, int s_dg,
                                           int s_act, int row0, int B, int od, int ad, int K0, int S, int tid) {
    const int K = od + 6 + ad;
    for (int idx = tid; idx < MT * 16 * K0; idx += THREADS) {
        const int r = idx / K0, k = idx - r * K0;
        const size_t b = (size_t)(row0 + r);
        float v = 0.0f;
        if (row0 + r < B && k < K) {
            if (k < 3) v = achieved_goal[b * s_ag + k];
            else if (k < 6) v = desired_goal[b * s_dg + (k - 3)];
            else if (k < 6 + od) v = obs[b * s_obs + (k - 6)];
            else v = action[b * s_act + (k - 6 - od)];
        }
        lds[r * S + k] = v;
    }
}

/* The sums of a batch row's log-probability, log_prob[b] = (lp_0 + lp_1 + ...) - (c_0 + c_1 + ...), each
 * from its first term in ascending d: thread (row r = tid / 8, dimension d = tid % 8) hands in its two
 * terms, the thread of d = 0 adds them up and stores.  sh: 512 floats of LDS.  Every thread of the
 * workgroup calls this (one barrier inside). */
__device__ __forceinline__ void sum_log_prob(float* sh, float lp, float c, bool own, int A, float* log_prob, size_t b,
                                             int tid) {
#pragma clang fp contract(off)
    sh[2 * tid] = lp;
    sh[2 * tid + 1] = c;
    __syncthreads();
    if (own && (tid & 7) == 0) {
        float s_lp = sh[2 * tid], s_c = sh[2 * tid + 1];
        for (int d = 1; d < A; d++) {
            s_lp = s_lp + sh[2 * (tid + d)];
            s_c = s_c + sh[2 * (tid + d) + 1];
        }
        log_prob[b] = s_lp - s_c;
    }
}

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

/* The first n Linears of plan p, a barrier behind each: lds[in_off..] (row stride s_in) -> region ping,
 * then ping and pong (row stride S) take turns as input and output.  ReLU on all but the last, on that
 * one too with relu_last.  Returns the LDS offset of the last output. */
template <int MT>
__device__ __forceinline__ int run_linears(float* lds, const float* params, const MlpPlan& p, int n, bool relu_last,
                                           int in_off, int s_in, int ping, int pong, int S, int lane, int wave) {
    int out_off = ping;
    for (int l = 0; l < n; l++) {
        linear_layer<MT>(lds, in_off, out_off, params + p.woff[l], params + p.boff[l], p.nkb[l], p.ntiles[l], s_in, S,
                         relu_last || l + 1 < n, lane, wave);
        __syncthreads();
        in_off = out_off;
        s_in = S;
        out_off = out_off == ping ? pong : ping;
    }
    return in_off;
}

/* Box-Muller's radius and angle from two Philox words: u1 in (0, 1], u2 in [0, 1) */
__device__ __forceinline__ void box_muller(uint32_t w0, uint32_t w1, float* rad, float* ang) {
    const float u1 = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-8f;
    const float u2 = (float)(w1 >> 8) * 5.9604644775390625e-8f;
    *rad = sqrtf(-2.0f * logf(u1));
    *ang = 6.2831855f * u2;
}

/* N(0, 1) for (env e, dimension d) at noise word `step`: dimensions 2 p and 2 p + 1 are the cosine and
 * the sine of block `tag ^ p`; the even one stores the block's words at philox_out (debug, or NULL) */
__device__ __forceinline__ float gaussian_draw(unsigned long long step, int e, int d, uint32_t tag, uint32_t seed_lo,
                                               uint32_t seed_hi, uint32_t* philox_out) {
    uint32_t rr[4];
    philox((uint32_t)step, (uint32_t)(step >> 32), (uint32_t)e, tag ^ (uint32_t)(d >> 1), seed_lo, seed_hi, rr);
    float rad, ang;
    box_muller(rr[0], rr[1], &rad, &ang);
    if (philox_out && (d & 1) == 0) {
        uint32_t* o = philox_out + ((size_t)e * 4 + (d >> 1)) * 4;
        o[0] = rr[0]; o[1] = rr[1]; o[2] = rr[2]; o[3] = rr[3];
    }
    return (d & 1) ? rad * sinf(ang) : rad * cosf(ang);
}

/* A 64-bit noise word on the device that one launch reads in every workgroup and moves on by one.
 * Thread 0 of each workgroup reads it into LDS (*sh) ahead of the workgroup's first barrier, so what
 * the workgroup computes behind that barrier uses the value read ... */
__device__ __forceinline__ void load_word(unsigned long long* sh, const unsigned long long* word, bool live, int tid) {
    if (tid == 0) *sh = live ? *word : 0ull;
}

/* ... and at its end takes a ticket.  Every one of the launch's n_groups workgroups has read the word
 * (ahead of its first barrier) by the time it takes its ticket: the last one to arrive moves the word
 * on and clears the ticket for the next launch, and no workgroup of this launch can see the new value. */
__device__ __forceinline__ void advance_word(unsigned long long* word, uint32_t* ticket, const unsigned long long* sh,
                                             uint32_t n_groups, bool live, int tid) {
    if (live && tid == 0) {
        __threadfence();
        if (atomicAdd(ticket, 1u) == n_groups - 1) {
            *ticket = 0u;
            *word = *sh + 1ull;
        }
    }
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
