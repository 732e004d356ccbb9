/*
 * pgx_actor.hip -- stable-baselines3's off-policy actor forward for gfx950, one launch.
 *
 * Restates the actor the reference trains (setup_training.py, hyperparameters.py: SB3
 * MultiInputPolicy, net_arch [256, 256] / [400, 300]): CombinedExtractor's concatenation in sorted
 * key order, the Linear + ReLU trunk, then SAC / TQC's squashed Gaussian (mu, log_std clamped to
 * [-20, 2], tanh) or TD3 / DDPG's tanh(mu) with NormalActionNoise and the clip.  Contract, noise
 * stream and packed weight layout: include/pgx.h, section "Actor".
 *
 * Forward kernel: a workgroup of 4 waves owns a tile of 16 (or 32) envs and keeps their
 * activations in LDS between layers, [env][feature] with a row stride of 4 floats past the widest
 * layer (the A reads of an MFMA step and the D stores both hit 64 distinct banks).  Every Linear
 * is v_mfma_f32_16x16x4_f32 with the envs on the A rows and 16 output features on the B columns:
 * wave w takes output tiles w, w + 4, ... four at a time, one accumulator each that starts at the
 * bias and takes every k step in ascending order -- no split of K, so a result is the fmaf chain
 * of the contract bit for bit.  Weights stream from global memory (L2 after the first workgroup)
 * as one 16-byte load per lane per 16 k, fetched one block ahead of the MFMAs that use them.  The
 * tail is masked: envs past N are staged as zero rows and never stored, the K remainder of the
 * input is staged as +0 against zero weights.
 * The staging, the Linear, the loop over the layers, the Gaussian draw and the noise step word's read
 * and advance are pgx_mlp.h's, shared with the other policy units; the epilogue is this unit's.  The
 * host-side plan, allocation and packing are pgx_policy.h's.
 *
 * Log-probability kernel (pgx_actor_action_log_prob, SB3's actor.action_log_prob): the same workgroup
 * over a tile of 32 batch rows (16 for a batch of up to 16, or where 32 do not fit the LDS), the batch
 * size a launch argument and every observation field read through its own row stride (pgx_mlp.h's
 * stage_rows).  Behind the head tile the thread of (row, dimension) computes the squashed action
 * and its two log-probability terms with contraction off; the terms go through the dead activations
 * and the thread of dimension 0 adds them in ascending order.  Its noise word is another than the
 * forward's.
 */
#include "pgx_policy.h"   /* pgx_mlp.h, pgx_common.h, include/pgx.h */

/* pgx_actor_host.cpp */
int pgx_actor_check_config(const pgx_actor_config* c, const char* what, bool with_envs);
int pgx_actor_lp_check_launch(const pgx_actor_config* c, const pgx_actor_lp_io* io, int32_t B, const char* what);

namespace {

constexpr uint32_t TAG_ACTOR = 0x41435430u;
constexpr int LOG_STD_ROW = 8;  /* the head tile: mu in rows 0..6, log_std in rows 8..14 */

struct ActorArgs {
    int32_t n, od, ad, kind, S;   /* S: LDS row stride (floats) */
    float clip, noise_mu, noise_sigma;
    uint32_t seed_lo, seed_hi;
    MlpPlan plan;                 /* the trunk and the head tile */
    const float* params;
    unsigned long long* step;
    uint32_t* ticket;
};

template <int MT>
__global__ __launch_bounds__(THREADS) void actor_forward_kernel(ActorArgs a, pgx_actor_io io, int32_t deterministic) {
    extern __shared__ float lds[];
    __shared__ unsigned long long sh_step;
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, N = a.n, od = a.od, A = a.ad;
    const int env0 = blockIdx.x * ROWS;
    const bool draw = deterministic == 0 && io.eps == nullptr;
    load_word(&sh_step, a.step, draw, tid);
    stage_features<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, env0, N, od, a.plan.nkb[0] * 16, S, tid);
    __syncthreads();
    /* the features lie in region 0; it and region ROWS * S take turns */
    const int in_off = run_linears<MT>(lds, a.params, a.plan, a.plan.n_linear, false, 0, S, ROWS * S, 0, S, lane, wave);
    /* epilogue: one thread per (env, dimension); the head tile lies at lds[in_off] */
    const int r = tid >> 3, d = tid & 7;
    const int e = env0 + r;
    if (r < ROWS && d < A && e < N) {
        const float* head = lds + in_off + r * S;
        float mean = head[d];
        if (a.clip > 0.0f) mean = mean < -a.clip ? -a.clip : (mean > a.clip ? a.clip : mean);
        float eps = 0.0f;
        if (deterministic == 0) {
            if (io.eps) eps = io.eps[(size_t)e * A + d];
            else eps = gaussian_draw(sh_step, e, d, TAG_ACTOR, a.seed_lo, a.seed_hi, io.philox_out);
        }
        float act;
        if (a.kind == PGX_ACTOR_GAUSSIAN) {
            const float v = head[LOG_STD_ROW + d];
            const float ls = v < PGX_ACTOR_LOG_STD_MIN ? PGX_ACTOR_LOG_STD_MIN : (v > PGX_ACTOR_LOG_STD_MAX ? PGX_ACTOR_LOG_STD_MAX : v);
            act = tanhf(deterministic != 0 ? mean : fmaf(expf(ls), eps, mean));
            if (io.log_std_out) io.log_std_out[(size_t)e * A + d] = ls;
        } else {
            act = tanhf(mean);
            if (deterministic == 0) act = act + fmaf(a.noise_sigma, eps, a.noise_mu);
            act = act < -1.0f ? -1.0f : (act > 1.0f ? 1.0f : act);
        }
        io.action[(size_t)e * A + d] = act;
        if (io.mean_out) io.mean_out[(size_t)e * A + d] = mean;
        if (io.eps_out) io.eps_out[(size_t)e * A + d] = eps;
    }
    advance_word(a.step, a.ticket, &sh_step, gridDim.x, draw, tid);
}

/* the log-probability epilogue of one (row, dimension), every operation rounded on its own but the fmaf */
__device__ __forceinline__ void lp_terms(float mean, float ls, float eps, float* g, float* act, float* lp, float* c) {
#pragma clang fp contract(off)
    const float std = expf(ls);
    *g = __builtin_fmaf(std, eps, mean);
    const float t = tanhf(*g);
    const float z = *g - mean;
    *lp = ((-(z * z)) / (2.0f * (std * std)) - ls) - 0.9189385f;
    *c = logf((1.0f - t * t) + 1e-6f);
    *act = t;
}

/* pgx_actor_action_log_prob: the forward's workgroup over a tile of batch rows read through their strides;
 * a.n is the batch size, a.step / a.ticket the log-probability noise word and its ticket */
template <int MT>
__global__ __launch_bounds__(THREADS) void actor_lp_kernel(ActorArgs a, pgx_actor_lp_io io) {
    extern __shared__ float lds[];
    __shared__ unsigned long long sh_step;
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, B = a.n, A = a.ad;
    const int row0 = blockIdx.x * ROWS;
    const bool draw = io.eps == nullptr;
    load_word(&sh_step, a.step, draw, tid);
    stage_rows<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, nullptr, io.obs_stride, io.achieved_goal_stride,
                   io.desired_goal_stride, 0, row0, B, a.od, 0, a.plan.nkb[0] * 16, S, tid);
    __syncthreads();
    const int in_off = run_linears<MT>(lds, a.params, a.plan, a.plan.n_linear, false, 0, S, ROWS * S, 0, S, lane, wave);
    /* one thread per (row, dimension); the head tile lies at lds[in_off] */
    const int r = tid >> 3, d = tid & 7;
    const int b = row0 + r;
    const bool own = r < ROWS && d < A && b < B;
    float lp = 0.0f, c = 0.0f;
    if (own) {
        const float* head = lds + in_off + r * S;
        float mean = head[d];
        if (a.clip > 0.0f) mean = mean < -a.clip ? -a.clip : (mean > a.clip ? a.clip : mean);
        const float v = head[LOG_STD_ROW + d];
        const float ls = v < PGX_ACTOR_LOG_STD_MIN ? PGX_ACTOR_LOG_STD_MIN : (v > PGX_ACTOR_LOG_STD_MAX ? PGX_ACTOR_LOG_STD_MAX : v);
        const size_t o = (size_t)b * A + d;
        const float eps = io.eps ? io.eps[o] : gaussian_draw(sh_step, b, d, PGX_ACTOR_LP_PHILOX_TAG, a.seed_lo, a.seed_hi, io.philox_out);
        float g, act;
        lp_terms(mean, ls, eps, &g, &act, &lp, &c);
        io.action[o] = act;
        if (io.mean_out) io.mean_out[o] = mean;
        if (io.log_std_out) io.log_std_out[o] = ls;
        if (io.eps_out) io.eps_out[o] = eps;
        if (io.gaussian_action_out) io.gaussian_action_out[o] = g;
    }
    __syncthreads();   /* the head tile is read: the activations are dead and carry the sums' terms */
    sum_log_prob(lds, lp, c, own, A, io.log_prob, (size_t)b, tid);
    advance_word(a.step, a.ticket, &sh_step, gridDim.x, draw, tid);
}

}  // namespace

struct pgx_actor {
    int device;
    pgx_actor_config cfg;
    ActorArgs a;
    float* params;              /* packed weights and padded biases; the head of the one allocation */
    float* plain;               /* the parameters as given, torch layout */
    size_t plain_w[5], plain_b[5];   /* per slot: the hidden layers, mu, log_std */
    int mt;                     /* env tiles of 16 per workgroup */
    size_t lds_bytes;
    unsigned long long* lp_step;   /* the log-probability noise word and its ticket, in the words' region */
    uint32_t* lp_ticket;

    size_t lds_need(int mt) const { return 2 * (size_t)mt * 16 * a.S * 4; }
    /* row tiles of 16 per workgroup of a batch launch: 32 rows from 17 on, where they fit the LDS */
    int lp_tile(int B) const {
        return choose_tile(B, "PGX_ACTOR_LP_TILE", [this](int mt) { return lds_need(mt); }, 17);
    }
};

extern "C" {

int pgx_actor_create(const pgx_actor_config* cfg, int device, pgx_actor_handle* out) {
    int rc = pgx_actor_check_config(cfg, "pgx_actor_create", true);
    if (rc != PGX_OK) return rc;
    if (!out) return pgx_set_error(PGX_E_INVALID, "pgx_actor_create: null handle pointer");
    *out = nullptr;
    pgx_actor* h = new pgx_actor();
    h->device = device;
    h->cfg = *cfg;
    ActorArgs& a = h->a;
    const int nl = cfg->n_layers;
    a.n = cfg->n_envs;
    a.od = cfg->obs_dim;
    a.ad = cfg->action_dim;
    a.kind = cfg->kind;
    a.clip = (float)cfg->clip_mean;
    a.noise_mu = (float)cfg->noise_mu;
    a.noise_sigma = (float)cfg->noise_sigma;
    a.seed_lo = (uint32_t)cfg->seed;
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    size_t n_params = 0, n_plain = 0;
    a.S = 4 + plan_stack(&a.plan, cfg->obs_dim + 6, cfg->hidden, nl, cfg->action_dim, 0, &n_params, h->plain_w,
                         h->plain_b, &n_plain);
    if (cfg->kind == PGX_ACTOR_GAUSSIAN) {   /* log_std: a plain slot more, packed into mu's tile */
        h->plain_w[nl + 1] = n_plain;
        n_plain += (size_t)cfg->action_dim * cfg->hidden[nl - 1];
        h->plain_b[nl + 1] = n_plain;
        n_plain += (size_t)cfg->action_dim;
    }
    auto lds_need = [&a](int mt) { return 2 * (size_t)mt * 16 * a.S * 4; };
    h->mt = choose_tile(cfg->n_envs, "PGX_ACTOR_TILE", lds_need);
    if (h->mt == 0) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_actor_create: obs_dim too wide for the activations in LDS");
    }
    h->lds_bytes = lds_need(h->mt);
    const size_t bytes[3] = {n_params * 4, n_plain * 4, 256};
    void* ptr[3];
    const void* fn = h->mt == 2 ? (const void*)actor_forward_kernel<2> : (const void*)actor_forward_kernel<1>;
    rc = create_blob("pgx_actor_create", device, bytes, 3, ptr, {fn}, h->lds_bytes);
    if (rc != PGX_OK) {
        delete h;
        return rc;
    }
    a.params = h->params = (float*)ptr[0];
    h->plain = (float*)ptr[1];
    a.step = (unsigned long long*)ptr[2];
    a.ticket = (uint32_t*)((char*)ptr[2] + 8);
    h->lp_step = (unsigned long long*)((char*)ptr[2] + 16);
    h->lp_ticket = (uint32_t*)((char*)ptr[2] + 24);
    if (cfg->kind == PGX_ACTOR_GAUSSIAN && !set_tile_lds(actor_lp_kernel<1>, actor_lp_kernel<2>, lds_need)) {
        (void)hipFree(h->params);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_actor_create: device setup failed");
    }
    *out = h;
    return PGX_OK;
}

void pgx_actor_destroy(pgx_actor_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->params);
    delete h;
}

int pgx_actor_set_weights(pgx_actor_handle h, const pgx_actor_weights* w, void* stream) {
    if (!h || !w) return pgx_set_error(PGX_E_INVALID, "pgx_actor_set_weights: null handle or weights");
    const int nl = h->cfg.n_layers, heads = h->cfg.kind == PGX_ACTOR_GAUSSIAN ? 2 : 1;
    for (int i = 0; i < nl + heads; i++)
        if (!w->weight[i] || !w->bias[i])
            return pgx_set_error(PGX_E_INVALID, "pgx_actor_set_weights: null weight or bias pointer");
    hipStream_t st = (hipStream_t)stream;
    const MlpPlan& p = h->a.plan;
    for (int i = 0; i < nl + heads; i++) {
        const int l = i < nl ? i : nl;   /* mu and log_std share the head tile */
        int o, in;
        linear_dims(h->cfg.obs_dim + 6, h->cfg.hidden, nl, h->cfg.action_dim, l, &o, &in);
        if (!pack_linear(w->weight[i], w->bias[i], h->plain + h->plain_w[i], h->plain + h->plain_b[i], o, in,
                         h->params + p.woff[l], h->params + p.boff[l], p.ntiles[l], i > nl ? LOG_STD_ROW : 0, st))
            return pgx_set_error(PGX_E_HIP, "pgx_actor_set_weights: copy failed");
    }
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_actor_set_weights: launch failed");
}

int pgx_actor_forward(pgx_actor_handle h, const pgx_actor_io* io, int32_t deterministic, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_actor_forward: null handle or io");
    if (!io->obs || !io->achieved_goal || !io->desired_goal || !io->action)
        return pgx_set_error(PGX_E_INVALID, "pgx_actor_forward: null observation or action pointer");
    launch_tiles(actor_forward_kernel<1>, actor_forward_kernel<2>, h->mt, h->a.n, h->lds_bytes, stream, h->a, *io,
                 deterministic);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_actor_forward: launch failed");
}

int pgx_actor_action_log_prob(pgx_actor_handle h, const pgx_actor_lp_io* io, int32_t B, void* stream) {
    const char* what = "pgx_actor_action_log_prob";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int rc = pgx_actor_lp_check_launch(&h->cfg, io, B, what);
    if (rc != PGX_OK) return rc;
    ActorArgs a = h->a;
    a.n = B;
    a.step = h->lp_step;
    a.ticket = h->lp_ticket;
    const int mt = h->lp_tile(B);
    launch_tiles(actor_lp_kernel<1>, actor_lp_kernel<2>, mt, B, h->lds_need(mt), stream, a, *io);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_actor_lp_state(pgx_actor_handle h, uint64_t* word, void* stream) {
    if (!h || !word) return pgx_set_error(PGX_E_INVALID, "pgx_actor_lp_state: null handle or word pointer");
    return read_word("pgx_actor_lp_state", h->lp_step, word, stream);
}

int pgx_actor_lp_set_state(pgx_actor_handle h, uint64_t word, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_actor_lp_set_state: null handle");
    return write_word("pgx_actor_lp_set_state", h->lp_step, word, stream);
}

int pgx_actor_state(pgx_actor_handle h, uint64_t* step, void* stream) {
    if (!h || !step) return pgx_set_error(PGX_E_INVALID, "pgx_actor_state: null handle or step pointer");
    return read_word("pgx_actor_state", h->a.step, step, stream);
}

int pgx_actor_set_state(pgx_actor_handle h, uint64_t step, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_actor_set_state: null handle");
    return write_word("pgx_actor_set_state", h->a.step, step, stream);
}

}  // extern "C"
