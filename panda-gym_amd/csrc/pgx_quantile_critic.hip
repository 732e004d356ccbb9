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
 */
#include "pgx_policy.h"   /* pgx_mlp.h, pgx_common.h, include/pgx.h */

/* pgx_actor_host.cpp */
int pgx_qc_check_config(const pgx_qc_config* c, const char* what);
int pgx_qc_check_launch(const pgx_qc_config* c, const pgx_qc_io* io, int32_t B, bool target, int32_t n_target,
                        const char* what);
int pgx_qc_check_weights(const pgx_qc_config* c, const pgx_qc_weights* w, const char* what);

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

/* features of the workgroup's MT x 16 rows into lds (row stride S0), K0 columns each: achieved_goal |
 * desired_goal | observation | action through their row strides, +0 past K and past row B */
template <int MT>
__device__ __forceinline__ void stage_rows(float* lds, const pgx_qc_io& io, int row0, int B, int od, int ad, int K0,
                                           int S0, int tid) {
    const int K = od + 6 + ad;
    for (int idx = tid; idx < MT * 16 * K0; idx += THREADS) {
        const int r = idx / K0, k = idx - r * K0;
        const size_t b = (size_t)(row0 + r);
        float v = 0.0f;
        if (row0 + r < B && k < K) {
            if (k < 3) v = io.achieved_goal[b * io.achieved_goal_stride + k];
            else if (k < 6) v = io.desired_goal[b * io.desired_goal_stride + (k - 3)];
            else if (k < 6 + od) v = io.obs[b * io.obs_stride + (k - 6)];
            else v = io.action[b * io.action_stride + (k - 6 - od)];
        }
        lds[r * S0 + k] = v;
    }
}

/* the rows' quantiles of every critic of the set at `params` into the pool region: critic c's quantile q
 * of row r at lds[ROWS * R0 + r * SP + c * HT * 16 + q]; ends behind a barrier */
template <int MT>
__device__ __forceinline__ void pooled_quantiles(float* lds, const QcArgs& a, const float* params, const pgx_qc_io& io,
                                                 int row0, int B, int tid) {
    constexpr int ROWS = MT * 16;
    const int lane = tid & 63, wave = tid >> 6;
    stage_rows<MT>(lds, io, row0, B, a.od, a.ad, a.plan.nkb[0] * 16, a.S0, tid);
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

}  // namespace

struct pgx_qc {
    int device;
    pgx_qc_config cfg;
    QcArgs a;
    float* params;              /* packed, [set][critic]; the head of the one allocation */
    float* plain;               /* the parameters as given, torch layout, [set][critic] */
    size_t plain_w[MAX_LINEAR], plain_b[MAX_LINEAR];   /* per Linear, floats from the critic's first */
    size_t critic_plain;        /* plain floats of one critic */

    size_t set_floats() const { return (size_t)cfg.n_critics * a.critic_floats; }
    size_t set_plain() const { return (size_t)cfg.n_critics * critic_plain; }
    size_t lds_need(int mt) const { return (size_t)mt * 16 * (a.R0 + a.SP) * 4; }
    int tile(int B) const {
        return choose_tile(B, "PGX_QC_TILE", [this](int mt) { return lds_need(mt); }, 17);
    }
};

namespace {

int bad_which(const char* what) { return fail(PGX_E_INVALID, what, "which must be PGX_QC_ONLINE or PGX_QC_TARGET"); }

/* packs set `which` from its plain copy, or (w != NULL) copies w's parameters there first */
bool pack_set(pgx_qc* h, int which, const pgx_qc_weights* w, hipStream_t st) {
    const MlpPlan& p = h->a.plan;
    const int nl = h->cfg.n_layers;
    for (int c = 0; c < h->cfg.n_critics; c++) {
        float* plain = h->plain + which * h->set_plain() + c * h->critic_plain;
        float* packed = h->params + which * h->set_floats() + (size_t)c * h->a.critic_floats;
        for (int l = 0; l <= nl; l++) {
            int o, in;
            linear_dims(h->cfg.obs_dim + 6 + h->cfg.action_dim, h->cfg.hidden, nl, h->cfg.n_quantiles, l, &o, &in);
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
    const int mt_max = choose_tile(17, nullptr, [h](int mt) { return h->lds_need(mt); }, 17);
    if (mt_max == 0) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_qc_create: obs_dim too wide for the features in LDS");
    }
    const size_t bytes[2] = {2 * h->set_floats() * 4, 2 * h->set_plain() * 4};
    void* ptr[2];
    const int rc = create_blob("pgx_qc_create", device, bytes, 2, ptr,
                               {(const void*)qc_forward_kernel<1>, (const void*)qc_forward_kernel<2>,
                                (const void*)qc_target_kernel<1>, (const void*)qc_target_kernel<2>},
                               h->lds_need(mt_max));
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
    delete h;
}

int pgx_qc_set_weights(pgx_qc_handle h, int32_t which, const pgx_qc_weights* w, void* stream) {
    const char* what = "pgx_qc_set_weights";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    if (which != PGX_QC_ONLINE && which != PGX_QC_TARGET) return bad_which(what);
    const int rc = pgx_qc_check_weights(&h->cfg, w, what);
    if (rc != PGX_OK) return rc;
    if (!pack_set(h, which, w, (hipStream_t)stream)) return fail(PGX_E_HIP, what, "copy failed");
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_get_weights(pgx_qc_handle h, int32_t which, const pgx_qc_weights* w, void* stream) {
    const char* what = "pgx_qc_get_weights";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    if (which != PGX_QC_ONLINE && which != PGX_QC_TARGET) return bad_which(what);
    const int rc = pgx_qc_check_weights(&h->cfg, w, what);
    if (rc != PGX_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nl = h->cfg.n_layers;
    for (int c = 0; c < h->cfg.n_critics; c++) {
        const float* plain = h->plain + which * h->set_plain() + c * h->critic_plain;
        for (int l = 0; l <= nl; l++) {
            int o, in;
            linear_dims(h->cfg.obs_dim + 6 + h->cfg.action_dim, h->cfg.hidden, nl, h->cfg.n_quantiles, l, &o, &in);
            if (hipMemcpyAsync(const_cast<float*>(w->weight[c][l]), plain + h->plain_w[l], (size_t)o * in * 4,
                               hipMemcpyDefault, st) != hipSuccess ||
                hipMemcpyAsync(const_cast<float*>(w->bias[c][l]), plain + h->plain_b[l], (size_t)o * 4, hipMemcpyDefault,
                               st) != hipSuccess)
                return fail(PGX_E_HIP, what, "copy failed");
        }
    }
    return hipStreamSynchronize(st) == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "synchronise failed");
}

int pgx_qc_forward(pgx_qc_handle h, int32_t which, const pgx_qc_io* io, int32_t B, void* stream) {
    const char* what = "pgx_qc_forward";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    if (which != PGX_QC_ONLINE && which != PGX_QC_TARGET) return bad_which(what);
    const int rc = pgx_qc_check_launch(&h->cfg, io, B, false, 0, what);
    if (rc != PGX_OK) return rc;
    const int mt = h->tile(B);
    const float* params = h->params + which * h->set_floats();
    launch_tiles(qc_forward_kernel<1>, qc_forward_kernel<2>, mt, B, h->lds_need(mt), stream, h->a, params, *io, B);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_qc_target(pgx_qc_handle h, const pgx_qc_io* io, int32_t B, int32_t n_target, void* stream) {
    const char* what = "pgx_qc_target";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int rc = pgx_qc_check_launch(&h->cfg, io, B, true, n_target, what);
    if (rc != PGX_OK) return rc;
    const int mt = h->tile(B);
    const float* params = h->params + PGX_QC_TARGET * h->set_floats();
    launch_tiles(qc_target_kernel<1>, qc_target_kernel<2>, mt, B, h->lds_need(mt), stream, h->a, params, *io, B,
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

}  // extern "C"
