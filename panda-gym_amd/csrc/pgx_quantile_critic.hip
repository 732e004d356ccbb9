/*
 * pgx_quantile_critic.hip -- sb3_contrib TQC's quantile critics for gfx950: the forward of `critic` or
 * `critic_target`, the truncated TD target of TQC.train's no_grad block as one launch, the Polyak step
 * and the hard copy.  Contract, order rule and packed weight layout: include/pgx.h, "QuantileCritic".
 *
 * A workgroup of 4 waves owns a tile of 32 batch rows (16 for a batch of up to 16, or where 32 do not fit
 * the LDS).  It stages their features once -- achieved_goal | desired_goal | observation | action, each
 * read through its own row stride, so the fields of a HER batch's rows are read where they lie -- into
 * an LDS region of their own, then runs the
 * critics one after the other: the hidden Linears through two activation regions (pgx_mlp.h's
 * run_linears, v_mfma_f32_16x16x4_f32, one accumulator per output from the bias on, k ascending), the
 * head of one or two tiles into the critic's columns of a pool region that holds the row's T = n_critics
 * * n_quantiles values.  The forward kernel stores the pool.  The target kernel turns it into the order
 * rule's integer keys, compact in the dead feature region, and ranks by counting: the thread of element
 * i counts the keys below its own, and the equal ones in front of it (four keys per LDS load), so the
 * ranks of a row are a permutation of 0 .. T - 1 for any input bits and every output slot below n_target is written exactly
 * once; the element whose rank is below n_target goes through the unfused backup and is stored.
 * Rows past B are staged as +0 and never stored.
 *
 * The critic update (include/pgx.h, "QuantileCritic, the critic update") is two more launches and Adam's.
 * qc_grad_rows_kernel is the forward's row tile again: it stores every activation to the caller's
 * workspace, turns the pool into dq and the loss terms, and walks the Linears backwards (linear_back: the
 * same MFMA loop against a transposed packing, accumulators from +0, the ReLU mask in the epilogue).
 * qc_wgrad_kernel gives one wave a 16 x 16 tile of one Linear's dW, chained over the batch four rows per
 * MFMA in ascending row order, the bias gradient beside it; its last workgroup adds up the loss.  No sum
 * is split and nothing is atomic, so the bits depend on the shapes alone.
 */
#include "pgx_policy.h"   /* pgx_mlp.h, pgx_common.h, include/pgx.h */

/* pgx_actor_host.cpp */
int pgx_qc_check_config(const pgx_qc_config* c, const char* what);
int pgx_qc_check_launch(const pgx_qc_config* c, const pgx_qc_io* io, int32_t B, bool target, int32_t n_target,
                        const char* what);
int pgx_qc_check_weights(const pgx_qc_config* c, const pgx_qc_weights* w, const char* what);
int pgx_qc_check_grad_launch(const pgx_qc_config* c, const pgx_qc_grad_io* io, int32_t B, int32_t n_target,
                             const char* what);
int pgx_qc_check_adam(double beta1, double beta2, double eps, const char* what);
float pgx_qc_inv_count(const pgx_qc_config* c, int32_t B, int32_t n_target);
int64_t pgx_qc_grad_row_floats(const pgx_qc_config* c);

namespace {

struct QcArgs {
    int32_t od, ad, nc, nq, T;
    int32_t S0, S, SP;            /* LDS row strides (floats): features, activations, pool */
    int32_t R0;                   /* floats per row of the region in front of the pool: max(S0 + 2 S, T up to 4) */
    int32_t HT;                   /* output tiles of the head */
    float gamma;
    int32_t critic_floats;        /* packed floats of one critic */
    MlpPlan plan;                 /* one critic's Linears, offsets from the critic's first float */
};

/* the rows' quantiles of every critic of the set at `params` into the pool region: critic c's quantile q
 * of row r at lds[ROWS * R0 + r * SP + c * HT * 16 + q]; ends behind a barrier */
template <int MT>
__device__ __forceinline__ void pooled_quantiles(float* lds, const QcArgs& a, const float* params, const pgx_qc_io& io,
                                                 int row0, int B, int tid) {
    constexpr int ROWS = MT * 16;
    const int lane = tid & 63, wave = tid >> 6;
    stage_rows<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, io.action, io.obs_stride, io.achieved_goal_stride,
                   io.desired_goal_stride, io.action_stride, row0, B, a.od, a.ad, a.plan.nkb[0] * 16, a.S0, tid);
    __syncthreads();
    const int ping = ROWS * a.S0, pong = ping + ROWS * a.S, pool = ROWS * a.R0;
    const int nl = a.plan.n_linear - 1;
    for (int c = 0; c < a.nc; c++) {
        const float* P = params + (size_t)c * a.critic_floats;
        const int in_off = run_linears<MT>(lds, P, a.plan, nl, true, 0, a.S0, ping, pong, a.S, lane, wave);
        linear_layer<MT>(lds, in_off, pool + c * a.HT * 16, P + a.plan.woff[nl], P + a.plan.boff[nl], a.plan.nkb[nl],
                         a.HT, a.S, a.SP, false, lane, wave);
        __syncthreads();
    }
}

template <int MT>
__global__ __launch_bounds__(THREADS) void qc_forward_kernel(QcArgs a, const float* params, pgx_qc_io io, int32_t B) {
    extern __shared__ float lds[];
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * ROWS;
    pooled_quantiles<MT>(lds, a, params, io, row0, B, tid);
    const float* pool = lds + ROWS * a.R0;
    for (int idx = tid; idx < ROWS * a.T; idx += THREADS) {
        const int r = idx / a.T, f = idx - r * a.T;
        const int c = f / a.nq, q = f - c * a.nq;
        if (row0 + r < B) io.out[(size_t)(row0 + r) * a.T + f] = pool[r * a.SP + c * a.HT * 16 + q];
    }
}

/* the order rule's key of an f32's bits, and back */
__device__ __forceinline__ uint32_t qc_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float qc_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

/* the epilogue of the truncated target, four operations, four roundings: the two a row's elements share ... */
__device__ __forceinline__ void qc_backup_row(float ent_coef, float next_log_prob, float done, float gamma, float* t1,
                                              float* m) {
#pragma clang fp contract(off)
    *t1 = ent_coef * next_log_prob;
    *m = (1.0f - done) * gamma;
}

/* ... and the two per element */
__device__ __forceinline__ float qc_backup(float z, float t1, float m, float reward) {
#pragma clang fp contract(off)
    const float t2 = z - t1;
    return reward + m * t2;
}

template <int MT>
__global__ __launch_bounds__(THREADS) void qc_target_kernel(QcArgs a, const float* params, pgx_qc_io io, int32_t B,
                                                            int32_t n_target) {
    extern __shared__ float lds[];
    __shared__ float row_t1[32], row_m[32], row_reward[32];   /* per row of the tile (384 of the 512 static bytes) */
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * ROWS;
    const int T = a.T;
    if (tid < ROWS && row0 + tid < B) {   /* read ahead of the Linears, used behind their barriers */
        const size_t b = (size_t)(row0 + tid);
        qc_backup_row(*io.ent_coef, io.next_log_prob[b], io.done[b * io.done_stride], a.gamma, &row_t1[tid], &row_m[tid]);
        row_reward[tid] = io.reward[b * io.reward_stride];
    }
    pooled_quantiles<MT>(lds, a, params, io, row0, B, tid);
    /* keys, compact [row][T4] (T rounded up to 4, the pad at the largest key, which nothing counts), over the
     * features and activations nobody reads any more */
    const int T4 = (T + 3) & ~3;
    const float* pool = lds + ROWS * a.R0;
    uint32_t* keys = reinterpret_cast<uint32_t*>(lds);
    for (int idx = tid; idx < ROWS * T4; idx += THREADS) {
        const int r = idx / T4, f = idx - r * T4;
        uint32_t key = 0xFFFFFFFFu;
        if (f < T) {
            const int c = f / a.nq, q = f - c * a.nq;
            const float v = pool[r * a.SP + c * a.HT * 16 + q];
            if (io.quantiles_out && row0 + r < B) io.quantiles_out[(size_t)(row0 + r) * T + f] = v;
            key = qc_key(v);
        }
        keys[idx] = key;
    }
    __syncthreads();
    for (int idx = tid; idx < ROWS * T; idx += THREADS) {
        const int r = idx / T, f = idx - r * T;
        const int b = row0 + r;
        if (b >= B) continue;
        const uint32_t mine = keys[r * T4 + f];
        const uint4* kr = reinterpret_cast<const uint4*>(keys + r * T4);   /* 16-byte aligned: T4 is a multiple of 4 */
        int rank = 0;   /* the elements that precede this one: smaller keys, and equal keys in front of it */
        for (int j = 0; j < T4; j += 4) {
            const uint4 k = kr[j >> 2];
            rank += (k.x < mine || (k.x == mine && j < f)) ? 1 : 0;
            rank += (k.y < mine || (k.y == mine && j + 1 < f)) ? 1 : 0;
            rank += (k.z < mine || (k.z == mine && j + 2 < f)) ? 1 : 0;
            rank += (k.w < mine || (k.w == mine && j + 3 < f)) ? 1 : 0;
        }
        if (rank < n_target)
            io.out[(size_t)b * n_target + rank] = qc_backup(qc_unkey(mine), row_t1[r], row_m[r], row_reward[r]);
    }
}

/* t = fmaf(tau, p, t * (1 - tau)), the product rounded first */
__global__ __launch_bounds__(256) void qc_polyak_kernel(const float* __restrict__ p, float* __restrict__ t, int n,
                                                        float tau, float one_minus_tau) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float keep = t[i] * one_minus_tau;
        t[i] = fmaf(tau, p[i], keep);
    }
}

/* two copies in one launch: the plain and the packed parameters, online -> target */
__global__ __launch_bounds__(256) void qc_copy_kernel(const float* __restrict__ s0, float* __restrict__ d0, int n0,
                                                      const float* __restrict__ s1, float* __restrict__ d1, int n1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n0) d0[i] = s0[i];
    else if (i < n0 + n1) d1[i - n0] = s1[i - n0];
}

/* ------------------------------------------------------------------ the critic update (include/pgx.h) */

/* What the gradient kernels need beside QcArgs.  Workspace row (floats): x [K16] | per critic: A_0 ..
 * A_{nl-1} [H16_l], dZ_0 .. dZ_nl [H16_l .. Q16] | the row's loss term and 15 spare. */
struct QcGradArgs {
    int32_t S;                    /* LDS row stride of the two activation regions: 4 + max(widest H16, Q16) */
    int32_t W;                    /* workspace floats per row */
    int32_t CW, sumH16;           /* workspace floats per critic; of its A planes */
    int32_t hid[3], sumH;         /* hidden widths as given, and their sum: dz_out's columns */
    int32_t nt;
    float inv_count;
    int32_t ptoff[MAX_LINEAR];    /* transposed packing of Linear l >= 1, floats from the critic's first */
    int32_t critic_pt;            /* its floats per critic */
    int32_t out[MAX_LINEAR], in[MAX_LINEAR];   /* torch shapes */
    int32_t pw[MAX_LINEAR], pb[MAX_LINEAR];    /* plain offsets from the critic's first float */
    int32_t critic_plain;
    int32_t tile0[MAX_LINEAR + 1];             /* first weight-gradient tile of Linear l within a critic */
};

__device__ __forceinline__ int ws_a(const QcArgs& a, const QcGradArgs& g, int c, int l) {
    int o = a.plan.nkb[0] * 16 + c * g.CW;
    for (int i = 0; i < l; i++) o += a.plan.ntiles[i] * 16;
    return o;
}

/* plain [out, in] weights into the packed layout of the TRANSPOSED Linear (in outputs, out inputs): what
 * dA = dZ W reads as linear_back's weights; the padding was zeroed at init and is never written */
__global__ __launch_bounds__(256) void pack_t_kernel(const float* __restrict__ W, float* PT, int out, int in, int ntiles_t) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= out * in) return;
    const int o = idx / in, k = idx - o * in;
    const int tile = k >> 4, j = k & 15, kb = o >> 4, s = (o >> 2) & 3, kq = o & 3;
    PT[((size_t)(kb * ntiles_t + tile) * 64 + kq * 16 + j) * 4 + s] = W[idx];
}

/* One backward Linear over the workgroup's MT x 16 rows: dA = dZ W as pgx_mlp.h's linear_layer computes a
 * Linear (P: the transposed packing; every accumulator from +0), then dZ_prev = A_prev > 0 ? dA : +0 with
 * A_prev read from the workspace, stored to LDS (the next backward Linear's input), to the workspace and
 * (non-NULL) to the debug plane.  Rows past B are computed (their dZ is +0) and never stored. */
template <int MT>
__device__ __forceinline__ void linear_back(float* lds, int in_off, int out_off, const float* __restrict__ P, int nkb,
                                            int ntiles, int S, float* ws, int W, int a_col, int dz_col, float* dz_out,
                                            int dz_w, int dz_dbg_col, int width, int row0, int B, int lane, int wave) {
    const int col = lane & 15, kq = lane >> 4;
    const f32x4* Pv = reinterpret_cast<const f32x4*>(P);
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t0 = wave; t0 < ntiles; t0 += WAVES * NACC) {
        f32x4 acc[NACC][MT];
        bool valid[NACC];
#pragma unroll
        for (int i = 0; i < NACC; i++) {
            valid[i] = t0 + WAVES * i < ntiles;   /* the same in every lane of the wave */
#pragma unroll
            for (int m = 0; m < MT; m++) acc[i][m] = zero4;
        }
        for (int kb = 0; kb < nkb; kb++) {
            f32x4 w[NACC];
#pragma unroll
            for (int i = 0; i < NACC; i++) w[i] = valid[i] ? Pv[(kb * ntiles + t0 + WAVES * i) * 64 + lane] : zero4;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                float a[MT];
#pragma unroll
                for (int m = 0; m < MT; m++) a[m] = lds[in_off + (m * 16 + col) * S + kb * 16 + 4 * s + kq];
#pragma unroll
                for (int i = 0; i < NACC; i++) {
                    if (!valid[i]) continue;
#pragma unroll
                    for (int m = 0; m < MT; m++)
                        acc[i][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], w[i][s], acc[i][m], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NACC; i++) {
            if (!valid[i]) continue;
            const int k = (t0 + WAVES * i) * 16 + col;
#pragma unroll
            for (int m = 0; m < MT; m++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = m * 16 + kq * 4 + r;
                    const bool live = row0 + row < B;
                    float* wrow = ws + (size_t)(row0 + row) * W;
                    const float act = live ? wrow[a_col + k] : 0.0f;
                    const float v = act > 0.0f ? acc[i][m][r] : 0.0f;
                    lds[out_off + row * S + k] = v;
                    if (live) {
                        wrow[dz_col + k] = v;
                        if (dz_out && k < width) dz_out[(size_t)(row0 + row) * dz_w + dz_dbg_col + k] = v;
                    }
                }
        }
    }
}

/* a region of the tile's rows, `width` columns at LDS row stride S, into workspace column `wcol` */
template <int MT>
__device__ __forceinline__ void store_plane(const float* lds, int off, int S, int width, float* ws, int W, int wcol,
                                            int row0, int B, int tid) {
    for (int idx = tid; idx < MT * 16 * width; idx += THREADS) {
        const int r = idx / width, k = idx - r * width;
        if (row0 + r < B) ws[(size_t)(row0 + r) * W + wcol + k] = lds[off + r * S + k];
    }
}

/* the two chains of one (row, critic, quantile) over the row's targets */
__device__ __forceinline__ void qc_huber_chains(float q, const float* __restrict__ t, int nt, float tau, float* lt,
                                                float* gs) {
#pragma clang fp contract(off)
    float a_l = 0.0f, a_g = 0.0f;
    for (int k = 0; k < nt; k++) {
        const float d = t[k] - q;
        const float w = fabsf(tau - (d < 0.0f ? 1.0f : 0.0f));
        const float ad = fabsf(d);
        const float huber = ad > 1.0f ? ad - 0.5f : (d * d) * 0.5f;
        const float clamp = d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d);
        a_l = fmaf(w, huber, a_l);
        a_g = fmaf(w, clamp, a_g);
    }
    *lt = a_l;
    *gs = a_g;
}

/* Rows: the forward of the online critics with every activation stored, dq and the loss terms from the
 * pool, then the Linears backwards; one workgroup per tile of MT x 16 rows. */
template <int MT>
__global__ __launch_bounds__(THREADS) void qc_grad_rows_kernel(QcArgs a, QcGradArgs g, const float* params,
                                                               const float* pt, pgx_qc_grad_io io, int32_t B) {
#pragma clang fp contract(off)
    extern __shared__ float lds[];
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * ROWS;
    const int K16 = a.plan.nkb[0] * 16, nl = a.plan.n_linear - 1, Q16 = a.HT * 16, W = g.W;
    float* ws = io.workspace;
    stage_rows<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, io.action, io.obs_stride, io.achieved_goal_stride,
                   io.desired_goal_stride, io.action_stride, row0, B, a.od, a.ad, K16, a.S0, tid);
    __syncthreads();
    store_plane<MT>(lds, 0, a.S0, K16, ws, W, 0, row0, B, tid);
    const int ping = ROWS * a.S0, pong = ping + ROWS * g.S, pool = ROWS * (a.S0 + 2 * g.S);
    for (int c = 0; c < a.nc; c++) {
        const float* P = params + (size_t)c * a.critic_floats;
        const float* PT = pt + (size_t)c * g.critic_pt;
        int in_off = 0, s_in = a.S0, out_off = ping;
        for (int l = 0; l < nl; l++) {
            linear_layer<MT>(lds, in_off, out_off, P + a.plan.woff[l], P + a.plan.boff[l], a.plan.nkb[l], a.plan.ntiles[l],
                             s_in, g.S, true, lane, wave);
            __syncthreads();
            store_plane<MT>(lds, out_off, g.S, a.plan.ntiles[l] * 16, ws, W, ws_a(a, g, c, l), row0, B, tid);
            in_off = out_off;
            s_in = g.S;
            out_off = out_off == ping ? pong : ping;
        }
        linear_layer<MT>(lds, in_off, pool + c * Q16, P + a.plan.woff[nl], P + a.plan.boff[nl], a.plan.nkb[nl], a.HT, s_in,
                         a.SP, false, lane, wave);
        __syncthreads();
        /* dq into the free activation region (the head's dZ), the loss term over q in the pool */
        const int dq_col = ws_a(a, g, c, nl) + g.sumH16;
        for (int idx = tid; idx < ROWS * Q16; idx += THREADS) {
            const int r = idx / Q16, j = idx - r * Q16;
            const int b = row0 + r;
            float dq = 0.0f;
            if (j < a.nq && b < B) {
                const float q = lds[pool + r * a.SP + c * Q16 + j];
                const float tau = ((float)j + 0.5f) / (float)a.nq;
                float lt, gs;
                qc_huber_chains(q, io.target_quantiles + (size_t)b * g.nt, g.nt, tau, &lt, &gs);
                dq = (-g.inv_count) * gs;
                lds[pool + r * a.SP + c * Q16 + j] = lt;
                const size_t o = (size_t)b * a.T + c * a.nq + j;
                if (io.quantiles_out) io.quantiles_out[o] = q;
                if (io.dq_out) io.dq_out[o] = dq;
            }
            lds[out_off + r * g.S + j] = dq;
            if (b < B) ws[(size_t)b * W + dq_col + j] = dq;
        }
        __syncthreads();
        int d_off = out_off, free_off = out_off == ping ? pong : ping;
        for (int l = nl; l >= 1; l--) {
            int dbg = c * g.sumH;
            for (int i = 0; i < l - 1; i++) dbg += g.hid[i];
            linear_back<MT>(lds, d_off, free_off, PT + g.ptoff[l], a.plan.ntiles[l], a.plan.nkb[l], g.S, ws, W,
                            ws_a(a, g, c, l - 1), ws_a(a, g, c, l - 1) + g.sumH16, io.dz_out, a.nc * g.sumH, dbg,
                            g.hid[l - 1], row0, B, lane, wave);
            __syncthreads();
            const int t = d_off;
            d_off = free_off;
            free_off = t;
        }
    }
    if (tid < ROWS && row0 + tid < B) {
        float rl = 0.0f;
        for (int c = 0; c < a.nc; c++)
            for (int j = 0; j < a.nq; j++) rl = rl + lds[pool + tid * a.SP + c * Q16 + j];
        ws[(size_t)(row0 + tid) * W + a.plan.nkb[0] * 16 + a.nc * g.CW] = rl;
    }
}

constexpr int WG_STEPS = 8;   /* MFMAs (of four rows) whose operands one load group fetches */

/* Weights: one wave per 16 x 16 tile of one Linear's dW, its accumulator chained over the batch four rows
 * per MFMA; the tile of k block 0 chains the bias gradient beside it against a column of ones.  The last
 * workgroup adds up the loss in the stated order. */
__global__ __launch_bounds__(64) void qc_wgrad_kernel(QcArgs a, QcGradArgs g, float* ws, float* grad, float* loss,
                                                      int32_t B) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
    const int nl = a.plan.n_linear - 1, W = g.W;
    const int per_critic = g.tile0[nl + 1];
    const int loss_col = a.plan.nkb[0] * 16 + a.nc * g.CW;
    if ((int)blockIdx.x == a.nc * per_critic) {
        const int nseg = (B + 63) / 64;
        for (int s = lane; s < nseg; s += 64) {
            float seg = 0.0f;
            const int end = s * 64 + 64 < B ? s * 64 + 64 : B;
            for (int b = s * 64; b < end; b++) seg = seg + ws[(size_t)b * W + loss_col];
            ws[(size_t)s * 64 * W + loss_col + 1] = seg;
        }
        __syncthreads();
        if (lane == 0) {
            float total = 0.0f;
            for (int s = 0; s < nseg; s++) total = total + ws[(size_t)s * 64 * W + loss_col + 1];
            *loss = total * g.inv_count;
        }
        return;
    }
    const int c = blockIdx.x / per_critic;
    int rem = blockIdx.x - c * per_critic, l = 0;
    while (rem >= g.tile0[l + 1]) l++;
    rem -= g.tile0[l];
    const int nkb = a.plan.nkb[l];
    const int ot = rem / nkb, kb = rem - ot * nkb;
    const bool with_bias = kb == 0;
    const float* zp = ws + ws_a(a, g, c, l) + g.sumH16 + ot * 16 + col;
    const float* ap = ws + (l == 0 ? 0 : ws_a(a, g, c, l - 1)) + kb * 16 + col;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f}, accb = acc;
    float z[WG_STEPS], x[WG_STEPS], zn[WG_STEPS] = {}, xn[WG_STEPS] = {};
    auto fetch = [&](int b0, float* zz, float* xx) {
#pragma unroll
        for (int s = 0; s < WG_STEPS; s++) {
            const int b = b0 + 4 * s + kq;
            const bool live = b < B;
            zz[s] = live ? zp[(size_t)b * W] : 0.0f;
            xx[s] = live ? ap[(size_t)b * W] : 0.0f;
        }
    };
    fetch(0, z, x);
    for (int b0 = 0; b0 < B; b0 += 4 * WG_STEPS) {
        if (b0 + 4 * WG_STEPS < B) fetch(b0 + 4 * WG_STEPS, zn, xn);
#pragma unroll
        for (int s = 0; s < WG_STEPS; s++) {
            if (b0 + 4 * s >= B) break;   /* the same in every lane: ceil(B / 4) instructions in all */
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(z[s], x[s], acc, 0, 0, 0);
            if (with_bias) {
                const float one = b0 + 4 * s + kq < B ? 1.0f : 0.0f;
                accb = __builtin_amdgcn_mfma_f32_16x16x4f32(z[s], one, accb, 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < WG_STEPS; s++) {
            z[s] = zn[s];
            x[s] = xn[s];
        }
    }
    float* gc = grad + (size_t)c * g.critic_plain;
    const int k = kb * 16 + col;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int o = ot * 16 + kq * 4 + r;
        if (o < g.out[l] && k < g.in[l]) gc[g.pw[l] + (size_t)o * g.in[l] + k] = acc[r];
        if (with_bias && col == 0 && o < g.out[l]) gc[g.pb[l] + o] = accb[r];
    }
}

/* the step word moved on, and the two constants every element of this step shares */
__global__ void qc_adam_prep_kernel(unsigned long long* step, const float* __restrict__ lr, float* consts, double beta1,
                                    double beta2) {
#pragma clang fp contract(off)
    const unsigned long long t = *step + 1ull;
    *step = t;
    double p1 = 1.0, p2 = 1.0, s1 = beta1, s2 = beta2;
    for (unsigned long long n = t; n; n >>= 1) {
        if (n & 1ull) {
            p1 = p1 * s1;
            p2 = p2 * s2;
        }
        s1 = s1 * s1;
        s2 = s2 * s2;
    }
    const float bc1 = (float)(1.0 - p1), bc2 = (float)(1.0 - p2);
    consts[0] = *lr / bc1;
    consts[1] = sqrtf(bc2);
}

__global__ __launch_bounds__(256) void qc_adam_kernel(float* __restrict__ p, const float* __restrict__ grad,
                                                      float* __restrict__ m, float* __restrict__ v, int n,
                                                      const float* __restrict__ consts, float omb1, float b2, float omb2,
                                                      float eps) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = grad[i];
    const float mi = m[i] + (gi - m[i]) * omb1;
    const float vi = v[i] * b2 + omb2 * (gi * gi);
    m[i] = mi;
    v[i] = vi;
    const float u = consts[0] * (mi / (sqrtf(vi) / consts[1] + eps));
    if (!(u == 0.0f)) p[i] = p[i] - u;
}

}  // namespace

struct pgx_qc {
    int device;
    pgx_qc_config cfg;
    QcArgs a;
    float* params;              /* packed, [set][critic]; the head of the one allocation */
    float* plain;               /* the parameters as given, torch layout, [set][critic] */
    size_t plain_w[MAX_LINEAR], plain_b[MAX_LINEAR];   /* per Linear, floats from the critic's first */
    size_t critic_plain;        /* plain floats of one critic */
    /* the training state (pgx_qc_init_training): one allocation of its own, headed by grad */
    QcGradArgs g;
    float* grad = nullptr;      /* torch layout, online set: [critic] as plain */
    float *exp_avg = nullptr, *exp_avg_sq = nullptr;
    float* pt = nullptr;        /* transposed packing of the online Linears l >= 1, [critic] */
    float* consts = nullptr;    /* this step's step_size and sqrt(bc2) */
    unsigned long long* step = nullptr;
    double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;

    size_t set_floats() const { return (size_t)cfg.n_critics * a.critic_floats; }
    size_t set_plain() const { return (size_t)cfg.n_critics * critic_plain; }
    /* LDS floats per row of a forward / target launch, and of the gradient's rows launch */
    int fwd_row() const { return a.R0 + a.SP; }
    int grad_row() const { return a.S0 + 2 * g.S + a.SP; }
};

namespace {

/* the dynamic LDS of mt x 16 rows of row_floats each, as a function of mt */
auto lds_need(int row_floats) {
    return [row_floats](int mt) { return (size_t)mt * 16 * row_floats * 4; };
}

/* row tiles of 16 per workgroup of a launch over B rows: 32 rows from 17 on, where they fit the LDS */
int row_tile(int B, int row_floats) { return choose_tile(B, "PGX_QC_TILE", lds_need(row_floats), 17); }

/* the opening of the entry points that take a set */
int check_which(const pgx_qc* h, int which, const char* what) {
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    if (which != PGX_QC_ONLINE && which != PGX_QC_TARGET)
        return fail(PGX_E_INVALID, what, "which must be PGX_QC_ONLINE or PGX_QC_TARGET");
    return PGX_OK;
}

/* packs set `which` from its plain copy, or (w != NULL) copies w's parameters there first */
bool pack_set(pgx_qc* h, int which, const pgx_qc_weights* w, hipStream_t st) {
    const MlpPlan& p = h->a.plan;
    const int nl = h->cfg.n_layers;
    for (int c = 0; c < h->cfg.n_critics; c++) {
        float* plain = h->plain + which * h->set_plain() + c * h->critic_plain;
        float* packed = h->params + which * h->set_floats() + (size_t)c * h->a.critic_floats;
        for (int l = 0; l <= nl; l++) {
            const int o = h->g.out[l], in = h->g.in[l];
            float* pw = plain + h->plain_w[l];
            float* pb = plain + h->plain_b[l];
            const bool ok = w ? pack_linear(w->weight[c][l], w->bias[c][l], pw, pb, o, in, packed + p.woff[l],
                                            packed + p.boff[l], p.ntiles[l], 0, st)
                              : pack_linear(pw, pb, nullptr, nullptr, o, in, packed + p.woff[l], packed + p.boff[l],
                                            p.ntiles[l], 0, st);
            if (!ok) return false;
        }
    }
    return true;
}

/* the online set's transposed packing from its plain copy (no-op before pgx_qc_init_training) */
void pack_transposed(pgx_qc* h, hipStream_t st) {
    if (!h->pt) return;
    for (int c = 0; c < h->cfg.n_critics; c++)
        for (int l = 1; l <= h->cfg.n_layers; l++) {
            const int n = h->g.out[l] * h->g.in[l];
            hipLaunchKernelGGL(pack_t_kernel, dim3((n + 255) / 256), dim3(256), 0, st,
                               h->plain + c * h->critic_plain + h->plain_w[l],
                               h->pt + (size_t)c * h->g.critic_pt + h->g.ptoff[l], h->g.out[l], h->g.in[l],
                               h->a.plan.nkb[l]);
        }
}

/* torch-layout floats of the handle at `base` ([critic] as plain) to (to_user) or from w's pointers */
bool copy_plain(pgx_qc* h, float* base, const pgx_qc_weights* w, bool to_user, hipStream_t st) {
    for (int c = 0; c < h->cfg.n_critics; c++)
        for (int l = 0; l <= h->cfg.n_layers; l++) {
            float* pw = base + c * h->critic_plain + h->plain_w[l];
            float* pb = base + c * h->critic_plain + h->plain_b[l];
            float* uw = const_cast<float*>(w->weight[c][l]);
            float* ub = const_cast<float*>(w->bias[c][l]);
            const size_t nw = (size_t)h->g.out[l] * h->g.in[l] * 4, nb = (size_t)h->g.out[l] * 4;
            if (hipMemcpyAsync(to_user ? uw : pw, to_user ? pw : uw, nw, hipMemcpyDefault, st) != hipSuccess ||
                hipMemcpyAsync(to_user ? ub : pb, to_user ? pb : ub, nb, hipMemcpyDefault, st) != hipSuccess)
                return false;
        }
    return true;
}

int need_training(const pgx_qc* h, const char* what) {
    return h->grad ? PGX_OK : fail(PGX_E_INVALID, what, "call pgx_qc_init_training first");
}

}  // namespace

extern "C" {

int pgx_qc_create(const pgx_qc_config* cfg, int device, pgx_qc_handle* out) {
    const int rc0 = pgx_qc_check_config(cfg, "pgx_qc_create");
    if (rc0 != PGX_OK) return rc0;
    if (!out) return pgx_set_error(PGX_E_INVALID, "pgx_qc_create: null handle pointer");
    *out = nullptr;
    pgx_qc* h = new pgx_qc();
    h->device = device;
    h->cfg = *cfg;
    QcArgs& a = h->a;
    a.od = cfg->obs_dim;
    a.ad = cfg->action_dim;
    a.nc = cfg->n_critics;
    a.nq = cfg->n_quantiles;
    a.T = cfg->n_critics * cfg->n_quantiles;
    a.gamma = (float)cfg->gamma;
    size_t n_params = 0, n_plain = 0;
    a.S = 4 + plan_stack(&a.plan, cfg->obs_dim + 6 + cfg->action_dim, cfg->hidden, cfg->n_layers, cfg->n_quantiles, 1,
                         &n_params, h->plain_w, h->plain_b, &n_plain);
    a.critic_floats = (int32_t)n_params;
    h->critic_plain = n_plain;
    a.S0 = a.plan.nkb[0] * 16 + 4;
    a.HT = a.plan.ntiles[cfg->n_layers];
    a.SP = a.nc * a.HT * 16 + 4;
    const int T4 = (a.T + 3) & ~3;
    a.R0 = a.S0 + 2 * a.S > T4 ? a.S0 + 2 * a.S : T4;
    QcGradArgs& g = h->g;
    g = QcGradArgs();
    g.S = a.S > a.HT * 16 + 4 ? a.S : a.HT * 16 + 4;
    g.W = (int32_t)pgx_qc_grad_row_floats(cfg);
    g.critic_plain = (int32_t)n_plain;
    for (int l = 0; l <= cfg->n_layers; l++) {
        int o, in;
        linear_dims(cfg->obs_dim + 6 + cfg->action_dim, cfg->hidden, cfg->n_layers, cfg->n_quantiles, l, &o, &in);
        g.out[l] = o;
        g.in[l] = in;
        g.pw[l] = (int32_t)h->plain_w[l];
        g.pb[l] = (int32_t)h->plain_b[l];
        g.tile0[l + 1] = g.tile0[l] + a.plan.ntiles[l] * a.plan.nkb[l];
        g.ptoff[l] = g.critic_pt;
        if (l >= 1) g.critic_pt += a.plan.ntiles[l] * a.plan.nkb[l] * 256;
        if (l < cfg->n_layers) {
            g.hid[l] = cfg->hidden[l];
            g.sumH += cfg->hidden[l];
            g.sumH16 += a.plan.ntiles[l] * 16;
        }
    }
    g.CW = 2 * g.sumH16 + a.HT * 16;
    const int mt_max = max_tile(lds_need(h->fwd_row()));
    if (mt_max == 0) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_qc_create: obs_dim too wide for the features in LDS");
    }
    const size_t bytes[2] = {2 * h->set_floats() * 4, 2 * h->set_plain() * 4};
    void* ptr[2];
    const int rc = create_blob("pgx_qc_create", device, bytes, 2, ptr,
                               {(const void*)qc_forward_kernel<1>, (const void*)qc_forward_kernel<2>,
                                (const void*)qc_target_kernel<1>, (const void*)qc_target_kernel<2>},
                               lds_need(h->fwd_row())(mt_max));
    if (rc != PGX_OK) {
        delete h;
        return rc;
    }
    h->params = (float*)ptr[0];
    h->plain = (float*)ptr[1];
    *out = h;
    return PGX_OK;
}

void pgx_qc_destroy(pgx_qc_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->params);
    if (h->grad) (void)hipFree(h->grad);
    delete h;
}

int pgx_qc_set_weights(pgx_qc_handle h, int32_t which, const pgx_qc_weights* w, void* stream) {
    const char* what = "pgx_qc_set_weights";
    int rc = check_which(h, which, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(&h->cfg, w, what);
    if (rc != PGX_OK) return rc;
    if (!pack_set(h, which, w, (hipStream_t)stream)) return fail(PGX_E_HIP, what, "copy failed");
    if (which == PGX_QC_ONLINE) pack_transposed(h, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_get_weights(pgx_qc_handle h, int32_t which, const pgx_qc_weights* w, void* stream) {
    const char* what = "pgx_qc_get_weights";
    int rc = check_which(h, which, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(&h->cfg, w, what);
    if (rc != PGX_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!copy_plain(h, h->plain + which * h->set_plain(), w, true, st)) return fail(PGX_E_HIP, what, "copy failed");
    return hipStreamSynchronize(st) == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "synchronise failed");
}

int pgx_qc_forward(pgx_qc_handle h, int32_t which, const pgx_qc_io* io, int32_t B, void* stream) {
    const char* what = "pgx_qc_forward";
    int rc = check_which(h, which, what);
    if (rc == PGX_OK) rc = pgx_qc_check_launch(&h->cfg, io, B, false, 0, what);
    if (rc != PGX_OK) return rc;
    const int mt = row_tile(B, h->fwd_row());
    const float* params = h->params + which * h->set_floats();
    launch_tiles(qc_forward_kernel<1>, qc_forward_kernel<2>, mt, B, lds_need(h->fwd_row())(mt), stream, h->a, params, *io,
                 B);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_target(pgx_qc_handle h, const pgx_qc_io* io, int32_t B, int32_t n_target, void* stream) {
    const char* what = "pgx_qc_target";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int rc = pgx_qc_check_launch(&h->cfg, io, B, true, n_target, what);
    if (rc != PGX_OK) return rc;
    const int mt = row_tile(B, h->fwd_row());
    const float* params = h->params + PGX_QC_TARGET * h->set_floats();
    launch_tiles(qc_target_kernel<1>, qc_target_kernel<2>, mt, B, lds_need(h->fwd_row())(mt), stream, h->a, params, *io, B,
                 n_target);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_polyak(pgx_qc_handle h, double tau, void* stream) {
    const char* what = "pgx_qc_polyak";
    if (!(tau >= 0.0 && tau <= 1.0)) return fail(PGX_E_INVALID, what, "tau must be in [0, 1]");
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)h->set_plain();
    hipLaunchKernelGGL(qc_polyak_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h->plain, h->plain + h->set_plain(), n,
                       (float)tau, (float)(1.0 - tau));
    pack_set(h, PGX_QC_TARGET, nullptr, st);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_sync_target(pgx_qc_handle h, void* stream) {
    const char* what = "pgx_qc_sync_target";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int n0 = (int)h->set_plain(), n1 = (int)h->set_floats();
    hipLaunchKernelGGL(qc_copy_kernel, dim3((n0 + n1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->plain,
                       h->plain + n0, n0, h->params, h->params + n1, n1);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_init_training(pgx_qc_handle h, double beta1, double beta2, double eps) {
    const char* what = "pgx_qc_init_training";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int rc0 = pgx_qc_check_adam(beta1, beta2, eps, what);
    if (rc0 != PGX_OK) return rc0;
    const size_t n = h->set_plain();
    if (!h->grad) {
        const int mt_max = max_tile(lds_need(h->grad_row()));
        if (mt_max == 0) return fail(PGX_E_UNSUPPORTED, what, "the critic is too wide for the backward's rows in LDS");
        const size_t bytes[6] = {n * 4, n * 4, n * 4, (size_t)h->cfg.n_critics * h->g.critic_pt * 4 + 4, 2 * 4, 8};
        void* ptr[6];
        const int rc = create_blob(what, h->device, bytes, 6, ptr,
                                   {(const void*)qc_grad_rows_kernel<1>, (const void*)qc_grad_rows_kernel<2>},
                                   lds_need(h->grad_row())(mt_max));
        if (rc != PGX_OK) return rc;
        h->grad = (float*)ptr[0];
        h->exp_avg = (float*)ptr[1];
        h->exp_avg_sq = (float*)ptr[2];
        h->pt = (float*)ptr[3];
        h->consts = (float*)ptr[4];
        h->step = (unsigned long long*)ptr[5];
    } else {
        if (hipSetDevice(h->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemset(h->exp_avg, 0, n * 4) != hipSuccess || hipMemset(h->exp_avg_sq, 0, n * 4) != hipSuccess ||
            hipMemset(h->step, 0, 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            return fail(PGX_E_HIP, what, "device setup failed");
    }
    h->beta1 = beta1;
    h->beta2 = beta2;
    h->eps = eps;
    pack_transposed(h, nullptr);
    return hipDeviceSynchronize() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "packing failed");
}

int pgx_qc_critic_grad(pgx_qc_handle h, const pgx_qc_grad_io* io, int32_t B, int32_t n_target, void* stream) {
    const char* what = "pgx_qc_critic_grad";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    int rc = pgx_qc_check_grad_launch(&h->cfg, io, B, n_target, what);
    if (rc == PGX_OK) rc = need_training(h, what);
    if (rc != PGX_OK) return rc;
    QcGradArgs g = h->g;
    g.nt = n_target;
    g.inv_count = pgx_qc_inv_count(&h->cfg, B, n_target);
    const int mt = row_tile(B, h->grad_row());
    launch_tiles(qc_grad_rows_kernel<1>, qc_grad_rows_kernel<2>, mt, B, lds_need(h->grad_row())(mt), stream, h->a, g,
                 (const float*)h->params, (const float*)h->pt, *io, B);
    const int blocks = h->cfg.n_critics * g.tile0[h->cfg.n_layers + 1] + 1;
    hipLaunchKernelGGL(qc_wgrad_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, h->a, g, io->workspace, h->grad,
                       io->loss, B);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_get_grads(pgx_qc_handle h, const pgx_qc_weights* w, void* stream) {
    const char* what = "pgx_qc_get_grads";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    int rc = pgx_qc_check_weights(&h->cfg, w, what);
    if (rc == PGX_OK) rc = need_training(h, what);
    if (rc != PGX_OK) return rc;
    if (!copy_plain(h, h->grad, w, true, (hipStream_t)stream)) return fail(PGX_E_HIP, what, "copy failed");
    return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "synchronise failed");
}

int pgx_qc_adam_step(pgx_qc_handle h, const float* lr, void* stream) {
    const char* what = "pgx_qc_adam_step";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    if (!lr) return fail(PGX_E_INVALID, what, "null lr");
    const int rc = need_training(h, what);
    if (rc != PGX_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)h->set_plain();
    hipLaunchKernelGGL(qc_adam_prep_kernel, dim3(1), dim3(1), 0, st, h->step, lr, h->consts, h->beta1, h->beta2);
    hipLaunchKernelGGL(qc_adam_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h->plain, (const float*)h->grad,
                       h->exp_avg, h->exp_avg_sq, n, (const float*)h->consts, (float)(1.0 - h->beta1), (float)h->beta2,
                       (float)(1.0 - h->beta2), (float)h->eps);
    pack_set(h, PGX_QC_ONLINE, nullptr, st);
    pack_transposed(h, st);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_get_opt_state(pgx_qc_handle h, const pgx_qc_weights* exp_avg, const pgx_qc_weights* exp_avg_sq,
                         uint64_t* step, void* stream) {
    const char* what = "pgx_qc_get_opt_state";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    int rc = pgx_qc_check_weights(&h->cfg, exp_avg, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(&h->cfg, exp_avg_sq, what);
    if (rc == PGX_OK && !step) rc = fail(PGX_E_INVALID, what, "null step");
    if (rc == PGX_OK) rc = need_training(h, what);
    if (rc != PGX_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!copy_plain(h, h->exp_avg, exp_avg, true, st) || !copy_plain(h, h->exp_avg_sq, exp_avg_sq, true, st))
        return fail(PGX_E_HIP, what, "copy failed");
    return read_word(what, h->step, step, stream);
}

int pgx_qc_set_opt_state(pgx_qc_handle h, const pgx_qc_weights* exp_avg, const pgx_qc_weights* exp_avg_sq,
                         uint64_t step, void* stream) {
    const char* what = "pgx_qc_set_opt_state";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    int rc = pgx_qc_check_weights(&h->cfg, exp_avg, what);
    if (rc == PGX_OK) rc = pgx_qc_check_weights(&h->cfg, exp_avg_sq, what);
    if (rc == PGX_OK) rc = need_training(h, what);
    if (rc != PGX_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipStreamSynchronize(st) != hipSuccess || !copy_plain(h, h->exp_avg, exp_avg, false, st) ||
        !copy_plain(h, h->exp_avg_sq, exp_avg_sq, false, st))
        return fail(PGX_E_HIP, what, "copy failed");
    return write_word(what, h->step, step, stream);
}

}  // extern "C"
