/*
 * pgx_actor_critic.hip -- stable-baselines3's on-policy ActorCriticPolicy forward for gfx950.
 *
 * Restates the policy PPO trains in the reference (setup_training.py, hyperparameters.py: SB3
 * MultiInputPolicy, net_arch dict(pi=[256, 256], vf=[256, 256]), ReLU): CombinedExtractor's
 * concatenation, MlpExtractor's two separate trunks, action_net, value_net and the diagonal Gaussian
 * with a state-independent log_std.  Contract, noise stream and packed layout: include/pgx.h,
 * section "ActorCritic"; the staging, the Linear, the loop over a trunk's layers, the Gaussian draw and the
 * noise step word are pgx_mlp.h's, the host-side plan, allocation and packing pgx_policy.h's, both shared
 * with the other policy units.
 *
 * One kernel template, two entries.  A workgroup of 4 waves owns a tile of 16 (or 32) envs.  It
 * stages their features once into an LDS region of their own (row stride: the first layer's K16 + 4
 * floats), then runs a trunk and its head through two activation regions (row stride: the widest
 * hidden layer's K16 + 4) that take turns as input and output; the features stay for the second
 * trunk.  The forward runs the policy trunk, keeps each (env, dimension)'s mean in a register, runs
 * the value trunk and ends in the epilogue; the values entry runs the value trunk alone, and with a
 * `need` mask a workgroup none of whose envs is flagged writes +0 and leaves (the decision is
 * __syncthreads_or's, the same in every thread).  Tail: envs past N are staged as zero rows and
 * never stored.
 */
#include "pgx_policy.h"   /* pgx_mlp.h, pgx_common.h, include/pgx.h */

int pgx_ac_check_config(const pgx_ac_config* c, const char* what, bool with_envs);  /* pgx_actor_host.cpp */

namespace {

constexpr int PI = 0, VF = 1;

struct AcArgs {
    int32_t n, od, ad;
    int32_t SX, S;                  /* LDS row strides (floats): the features, the activations */
    uint32_t seed_lo, seed_hi;
    MlpPlan plan[2];                /* per trunk: hidden layers + head */
    int32_t ls_off;                 /* log_std [8], floats into params */
    const float* params;
    unsigned long long* step;
    uint32_t* ticket;
};

/* torch Normal.log_prob's order, every operation rounded on its own */
__device__ __forceinline__ float log_density(float z, float std, float log_std) {
#pragma clang fp contract(off)
    const float var = std * std;
    const float q = (-(z * z)) / (2.0f * var);
    return (q - log_std) - 0.9189385f;
}

/* trunk t and its head over the staged features; returns the LDS offset of the head tile */
template <int MT>
__device__ __forceinline__ int run_trunk(const AcArgs& a, float* lds, int t, int lane, int wave) {
    constexpr int ROWS = MT * 16;
    const int ping = ROWS * a.SX;   /* behind the features, which stay */
    return run_linears<MT>(lds, a.params, a.plan[t], a.plan[t].n_linear, false, 0, a.SX, ping, ping + ROWS * a.S, a.S,
                           lane, wave);
}

template <int MT, bool VALUES>
__global__ __launch_bounds__(THREADS) void ac_kernel(AcArgs a, pgx_ac_io io, const uint8_t* __restrict__ need,
                                                     int32_t deterministic) {
    extern __shared__ float lds[];
    __shared__ unsigned long long sh_step;
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.n, od = a.od, A = a.ad, SX = a.SX;
    const int env0 = blockIdx.x * ROWS;
    if (VALUES && need) {   /* a tile without a flagged env: +0 and done */
        const int flag = (tid < ROWS && env0 + tid < N) ? (need[env0 + tid] != 0) : 0;
        if (!__syncthreads_or(flag)) {
            if (tid < ROWS && env0 + tid < N) io.value[env0 + tid] = 0.0f;
            return;
        }
    }
    const bool draw = !VALUES && deterministic == 0 && io.eps == nullptr;
    load_word(&sh_step, a.step, draw, tid);
    /* (both trunks' first Linear has the K staged here) */
    stage_features<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, env0, N, od, a.plan[PI].nkb[0] * 16, SX, tid);
    __syncthreads();
    /* one thread per (env, dimension) */
    const int r = tid >> 3, d = tid & 7;
    const int e = env0 + r;
    const bool mine = r < ROWS && e < N;
    float mean = 0.0f;
    if (!VALUES) {
        const int head = run_trunk<MT>(a, lds, PI, lane, wave);
        if (r < ROWS && d < A) mean = lds[head + r * a.S + d];
        __syncthreads();   /* the value trunk writes where the head tile may lie */
    }
    const int vhead = run_trunk<MT>(a, lds, VF, lane, wave);
    if (mine && d == 0 && io.value) io.value[e] = lds[vhead + r * a.S];
    if (VALUES) return;
    /* epilogue; the features' region is free now: lp_d goes there, [ROWS][8] */
    float lp = 0.0f;
    if (mine && d < A) {
        float eps = 0.0f;
        if (deterministic == 0) {
            if (io.eps) eps = io.eps[(size_t)e * A + d];
            else eps = gaussian_draw(sh_step, e, d, PGX_AC_PHILOX_TAG, a.seed_lo, a.seed_hi, io.philox_out);
        }
        const float log_std = a.params[a.ls_off + d];
        const float std = expf(log_std);
        const float act = deterministic != 0 ? mean : fmaf(std, eps, mean);
        const float z = act - mean;
        lp = log_density(z, std, log_std);
        if (io.action) io.action[(size_t)e * A + d] = act;
        if (io.clipped_action) io.clipped_action[(size_t)e * A + d] = act < -1.0f ? -1.0f : (act > 1.0f ? 1.0f : act);
        if (io.mean_out) io.mean_out[(size_t)e * A + d] = mean;
        if (io.eps_out) io.eps_out[(size_t)e * A + d] = eps;
    }
    if (r < ROWS) lds[r * 8 + d] = lp;   /* ROWS * 8 <= ROWS * SX */
    __syncthreads();
    if (mine && d == 0 && io.log_prob) {
        float s = lds[r * 8];
        for (int j = 1; j < A; j++) s = s + lds[r * 8 + j];
        io.log_prob[e] = s;
    }
    advance_word(a.step, a.ticket, &sh_step, gridDim.x, draw, tid);
}

/* log_std into the packed parameters */
__global__ __launch_bounds__(64) void copy_kernel(const float* __restrict__ src, float* dst, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
}

constexpr int N_SLOTS = 2 * PGX_ACTOR_MAX_LAYERS + 2;   /* plain copies: pi layers, action_net, vf layers, value_net */

}  // namespace

struct pgx_ac {
    int device;
    pgx_ac_config cfg;
    AcArgs a;
    float* params;              /* packed weights, padded biases, log_std; the head of the one allocation */
    float* plain;               /* staging for parameters given as host pointers, torch layout */
    size_t plain_w[N_SLOTS], plain_b[N_SLOTS], plain_ls;
    int mt;                     /* env tiles of 16 per workgroup */
    size_t lds_bytes;
};

namespace {

/* trunk t of the config: its hidden widths and the width of its head */
const int32_t* trunk_dims(const pgx_ac_config& c, int t, int* nl, int* head_out) {
    *nl = t == PI ? c.n_pi_layers : c.n_vf_layers;
    *head_out = t == PI ? c.action_dim : 1;
    return t == PI ? c.pi_hidden : c.vf_hidden;
}

bool on_device(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();   /* an unregistered host pointer: not an error here */
        return false;
    }
    return at.type == hipMemoryTypeDevice;
}

size_t lds_need(const AcArgs& a, int mt) { return ((size_t)mt * 16 * a.SX + 2 * (size_t)mt * 16 * a.S) * 4; }

}  // namespace

extern "C" {

int pgx_ac_create(const pgx_ac_config* cfg, int device, pgx_ac_handle* out) {
    int rc = pgx_ac_check_config(cfg, "pgx_ac_create", true);
    if (rc != PGX_OK) return rc;
    if (!out) return pgx_set_error(PGX_E_INVALID, "pgx_ac_create: null handle pointer");
    *out = nullptr;
    pgx_ac* h = new pgx_ac();
    h->device = device;
    h->cfg = *cfg;
    AcArgs& a = h->a;
    a.n = cfg->n_envs;
    a.od = cfg->obs_dim;
    a.ad = cfg->action_dim;
    a.seed_lo = (uint32_t)cfg->seed;
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    size_t n_params = 0, n_plain = 0;
    int widest = 16, slot = 0;
    for (int t = 0; t < 2; t++) {
        int nl, head_out;
        const int32_t* hidden = trunk_dims(*cfg, t, &nl, &head_out);
        /* the activations are the inputs of l > 0: the features have a region and a stride of their own */
        const int w = plan_stack(&a.plan[t], cfg->obs_dim + 6, hidden, nl, head_out, 1, &n_params, h->plain_w + slot,
                                 h->plain_b + slot, &n_plain);
        if (w > widest) widest = w;
        slot += nl + 1;
    }
    a.ls_off = (int32_t)n_params;
    n_params += 8;
    h->plain_ls = n_plain;
    n_plain += 8;
    a.SX = a.plan[PI].nkb[0] * 16 + 4;
    a.S = widest + 4;
    /* the tile as the Actor chooses it, where the three regions fit */
    h->mt = choose_tile(cfg->n_envs, "PGX_AC_TILE", [&a](int mt) { return lds_need(a, mt); });
    if (h->mt == 0) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_ac_create: obs_dim too wide for the features in LDS");
    }
    h->lds_bytes = lds_need(a, h->mt);
    const size_t bytes[3] = {n_params * 4, n_plain * 4, 256};
    void* ptr[3];
    const void* fwd = h->mt == 2 ? (const void*)ac_kernel<2, false> : (const void*)ac_kernel<1, false>;
    const void* val = h->mt == 2 ? (const void*)ac_kernel<2, true> : (const void*)ac_kernel<1, true>;
    rc = create_blob("pgx_ac_create", device, bytes, 3, ptr, {fwd, val}, h->lds_bytes);
    if (rc != PGX_OK) {
        delete h;
        return rc;
    }
    a.params = h->params = (float*)ptr[0];
    h->plain = (float*)ptr[1];
    a.step = (unsigned long long*)ptr[2];
    a.ticket = (uint32_t*)((char*)ptr[2] + 8);
    *out = h;
    return PGX_OK;
}

void pgx_ac_destroy(pgx_ac_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->params);
    delete h;
}

int pgx_ac_set_weights(pgx_ac_handle h, const pgx_ac_weights* w, void* stream) {
    if (!h || !w) return pgx_set_error(PGX_E_INVALID, "pgx_ac_set_weights: null handle or weights");
    const float* W[2][MAX_LINEAR];
    const float* B[2][MAX_LINEAR];
    for (int t = 0; t < 2; t++) {
        const int nl = h->a.plan[t].n_linear - 1;
        for (int l = 0; l < nl; l++) {
            W[t][l] = t == PI ? w->pi_weight[l] : w->vf_weight[l];
            B[t][l] = t == PI ? w->pi_bias[l] : w->vf_bias[l];
        }
        W[t][nl] = t == PI ? w->action_net_weight : w->value_net_weight;
        B[t][nl] = t == PI ? w->action_net_bias : w->value_net_bias;
        for (int l = 0; l <= nl; l++)
            if (!W[t][l] || !B[t][l])
                return pgx_set_error(PGX_E_INVALID, "pgx_ac_set_weights: null weight or bias pointer");
    }
    if (!w->log_std) return pgx_set_error(PGX_E_INVALID, "pgx_ac_set_weights: null log_std pointer");
    hipStream_t st = (hipStream_t)stream;
    int slot = 0;
    for (int t = 0; t < 2; t++) {
        int nl, head_out, o, in;
        const int32_t* hidden = trunk_dims(h->cfg, t, &nl, &head_out);
        const MlpPlan& p = h->a.plan[t];
        for (int l = 0; l <= nl; l++, slot++) {
            linear_dims(h->cfg.obs_dim + 6, hidden, nl, head_out, l, &o, &in);
            /* device parameters are packed where they lie: launches only.  Host ones pass through the
             * handle's staging copy first */
            const bool stage = !on_device(W[t][l]) || !on_device(B[t][l]);
            if (!pack_linear(W[t][l], B[t][l], stage ? h->plain + h->plain_w[slot] : nullptr,
                             stage ? h->plain + h->plain_b[slot] : nullptr, o, in, h->params + p.woff[l],
                             h->params + p.boff[l], p.ntiles[l], 0, st))
                return pgx_set_error(PGX_E_HIP, "pgx_ac_set_weights: copy failed");
        }
    }
    const float* ls = w->log_std;
    if (!on_device(ls)) {
        if (hipMemcpyAsync(h->plain + h->plain_ls, ls, (size_t)h->a.ad * 4, hipMemcpyDefault, st) != hipSuccess)
            return pgx_set_error(PGX_E_HIP, "pgx_ac_set_weights: copy failed");
        ls = h->plain + h->plain_ls;
    }
    hipLaunchKernelGGL(copy_kernel, dim3(1), dim3(64), 0, st, ls, h->params + h->a.ls_off, h->a.ad);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_ac_set_weights: launch failed");
}

int pgx_ac_forward(pgx_ac_handle h, const pgx_ac_io* io, int32_t deterministic, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_ac_forward: null handle or io");
    if (!io->obs || !io->achieved_goal || !io->desired_goal)
        return pgx_set_error(PGX_E_INVALID, "pgx_ac_forward: null observation pointer");
    launch_tiles(ac_kernel<1, false>, ac_kernel<2, false>, h->mt, h->a.n, h->lds_bytes, stream, h->a, *io,
                 (const uint8_t*)nullptr, deterministic);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_ac_forward: launch failed");
}

int pgx_ac_values(pgx_ac_handle h, const float* obs, const float* achieved_goal, const float* desired_goal,
                  const uint8_t* need, float* value_out, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_ac_values: null handle");
    if (!obs || !achieved_goal || !desired_goal || !value_out)
        return pgx_set_error(PGX_E_INVALID, "pgx_ac_values: null observation or value pointer");
    pgx_ac_io io = {};
    io.obs = obs;
    io.achieved_goal = achieved_goal;
    io.desired_goal = desired_goal;
    io.value = value_out;
    launch_tiles(ac_kernel<1, true>, ac_kernel<2, true>, h->mt, h->a.n, h->lds_bytes, stream, h->a, io, need, (int32_t)1);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_ac_values: launch failed");
}

int pgx_ac_state(pgx_ac_handle h, uint64_t* step, void* stream) {
    if (!h || !step) return pgx_set_error(PGX_E_INVALID, "pgx_ac_state: null handle or step pointer");
    return read_word("pgx_ac_state", h->a.step, step, stream);
}

int pgx_ac_set_state(pgx_ac_handle h, uint64_t step, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_ac_set_state: null handle");
    return write_word("pgx_ac_set_state", h->a.step, step, stream);
}

}  // extern "C"
