/*
 * pgx_actor_critic.hip -- stable-baselines3's on-policy ActorCriticPolicy forward for gfx950.
 *
 * Restates the policy PPO trains in the reference (setup_training.py, hyperparameters.py: SB3
 * MultiInputPolicy, net_arch dict(pi=[256, 256], vf=[256, 256]), ReLU): CombinedExtractor's
 * concatenation, MlpExtractor's two separate trunks, action_net, value_net and the diagonal Gaussian
 * with a state-independent log_std.  Contract, noise stream and packed layout: include/pgx.h,
 * section "ActorCritic"; the Linear itself is pgx_mlp.h's, shared with the Actor.
 *
 * One kernel template, two entries.  A workgroup of 4 waves owns a tile of 16 (or 32) envs.  It
 * stages their features once into an LDS region of their own (row stride: the first layer's K16 + 4
 * floats), then runs a trunk and its head through two activation regions (row stride: the widest
 * hidden layer's K16 + 4) that take turns as input and output; the features stay for the second
 * trunk.  The forward runs the policy trunk, keeps each (env, dimension)'s mean in a register, runs
 * the value trunk and ends in the epilogue; the values entry runs the value trunk alone, and with a
 * `need` mask a workgroup none of whose envs is flagged writes +0 and leaves (the decision is
 * __syncthreads_or's, the same in every thread).  Tail: envs past N are staged as zero rows and
 * never stored.  The noise step word moves as the Actor's does.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "../../include/pgx.h"
#include "pgx_common.h"
#include "pgx_mlp.h"

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */
int pgx_ac_check_config(const pgx_ac_config* c, const char* what, bool with_envs);  /* pgx_actor_host.cpp */

namespace {

constexpr int THREADS = 64 * WAVES;
constexpr int MAX_LINEAR = PGX_ACTOR_MAX_LAYERS + 1;   /* the hidden layers and the head tile */
constexpr int PI = 0, VF = 1;

struct AcArgs {
    int32_t n, od, ad;
    int32_t SX, S;                  /* LDS row strides (floats): the features, the activations */
    uint32_t seed_lo, seed_hi;
    int32_t n_linear[2];            /* per trunk: hidden layers + head */
    int32_t nkb[2][MAX_LINEAR], ntiles[2][MAX_LINEAR];   /* 16-wide k blocks and output tiles per Linear */
    int32_t woff[2][MAX_LINEAR], boff[2][MAX_LINEAR];    /* packed weights / padded bias, floats into params */
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
    const int ping = ROWS * a.SX, pong = ping + ROWS * a.S;
    int in_off = 0, s_in = a.SX, out_off = ping;
    const int nl = a.n_linear[t];
    for (int l = 0; l < nl; l++) {
        linear_layer<MT>(lds, in_off, out_off, a.params + a.woff[t][l], a.params + a.boff[t][l], a.nkb[t][l],
                         a.ntiles[t][l], s_in, a.S, l + 1 < nl, lane, wave);
        __syncthreads();
        in_off = out_off;
        s_in = a.S;
        out_off = out_off == ping ? pong : ping;
    }
    return in_off;
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
    if (tid == 0) sh_step = draw ? *a.step : 0ull;
    /* features: achieved_goal | desired_goal | observation, +0 past in_dim and past env N */
    const int K0 = a.nkb[PI][0] * 16, in_dim = od + 6;   /* (both trunks' first Linear has this K) */
    for (int idx = tid; idx < ROWS * K0; idx += THREADS) {
        const int r = idx / K0, k = idx - r * K0;
        const int e = env0 + r;
        float v = 0.0f;
        if (e < N && k < in_dim) {
            if (k < 3) v = io.achieved_goal[(size_t)e * 3 + k];
            else if (k < 6) v = io.desired_goal[(size_t)e * 3 + (k - 3)];
            else v = io.obs[(size_t)e * od + (k - 6)];
        }
        lds[r * SX + k] = v;
    }
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
            if (io.eps) {
                eps = io.eps[(size_t)e * A + d];
            } else {
                const unsigned long long step = sh_step;
                uint32_t rr[4];
                philox((uint32_t)step, (uint32_t)(step >> 32), (uint32_t)e, PGX_AC_PHILOX_TAG ^ (uint32_t)(d >> 1),
                       a.seed_lo, a.seed_hi, rr);
                const float u1 = (float)((rr[0] >> 8) + 1u) * 5.9604644775390625e-8f;
                const float u2 = (float)(rr[1] >> 8) * 5.9604644775390625e-8f;
                const float rad = sqrtf(-2.0f * logf(u1)), ang = 6.2831855f * u2;
                eps = (d & 1) ? rad * sinf(ang) : rad * cosf(ang);
                if (io.philox_out && (d & 1) == 0) {
                    uint32_t* o = io.philox_out + ((size_t)e * 4 + (d >> 1)) * 4;
                    o[0] = rr[0]; o[1] = rr[1]; o[2] = rr[2]; o[3] = rr[3];
                }
            }
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
    /* every workgroup has read the step word (ahead of its first barrier): the last one to arrive
     * moves it on */
    if (draw && tid == 0) {
        __threadfence();
        if (atomicAdd(a.ticket, 1u) == gridDim.x - 1) {
            *a.ticket = 0u;
            *a.step = sh_step + 1ull;
        }
    }
}

/* log_std into the packed parameters */
__global__ __launch_bounds__(64) void copy_kernel(const float* __restrict__ src, float* dst, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x];
}

constexpr size_t LDS_LIMIT = 160 * 1024 - 512;   /* the Actor's 160 KB less the kernels' static words */
constexpr int N_SLOTS = 2 * PGX_ACTOR_MAX_LAYERS + 2;   /* plain copies: pi layers, action_net, vf layers, value_net */

}  // namespace

struct pgx_ac {
    int device;
    pgx_ac_config cfg;
    AcArgs a;
    void* blob;
    float* params;              /* packed weights, padded biases, log_std */
    float* plain;               /* staging for parameters given as host pointers, torch layout */
    size_t plain_w[N_SLOTS], plain_b[N_SLOTS], plain_ls;
    int mt;                     /* env tiles of 16 per workgroup */
    size_t lds_bytes;
};

namespace {

/* (out, in) of Linear l of trunk t: the hidden layers, then the head */
void linear_dims(const pgx_ac_config& c, int t, int l, int* out, int* in) {
    const int nl = t == PI ? c.n_pi_layers : c.n_vf_layers;
    const int32_t* hidden = t == PI ? c.pi_hidden : c.vf_hidden;
    *in = l == 0 ? c.obs_dim + 6 : hidden[l - 1];
    *out = l < nl ? hidden[l] : (t == PI ? c.action_dim : 1);
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

template <bool VALUES>
void launch(pgx_ac* h, const pgx_ac_io& io, const uint8_t* need, int32_t deterministic, hipStream_t st) {
    const int rows = h->mt * 16;
    const dim3 grid((h->a.n + rows - 1) / rows);
    if (h->mt == 2)
        hipLaunchKernelGGL((ac_kernel<2, VALUES>), grid, dim3(THREADS), h->lds_bytes, st, h->a, io, need, deterministic);
    else
        hipLaunchKernelGGL((ac_kernel<1, VALUES>), grid, dim3(THREADS), h->lds_bytes, st, h->a, io, need, deterministic);
}

}  // namespace

extern "C" {

int pgx_ac_create(const pgx_ac_config* cfg, int device, pgx_ac_handle* out) {
    const int rc = pgx_ac_check_config(cfg, "pgx_ac_create", true);
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
    size_t off = 0, n_plain = 0;
    int widest = 16, slot = 0;
    for (int t = 0; t < 2; t++) {
        const int nl = t == PI ? cfg->n_pi_layers : cfg->n_vf_layers;
        a.n_linear[t] = nl + 1;
        for (int l = 0; l <= nl; l++, slot++) {
            int o, in;
            linear_dims(*cfg, t, l, &o, &in);
            a.nkb[t][l] = (in + 15) / 16;
            a.ntiles[t][l] = l < nl ? (o + 15) / 16 : 1;
            a.woff[t][l] = (int32_t)off;
            off += (size_t)a.nkb[t][l] * a.ntiles[t][l] * 256;
            a.boff[t][l] = (int32_t)off;
            off += (size_t)a.ntiles[t][l] * 16;
            if (l > 0 && a.nkb[t][l] * 16 > widest) widest = a.nkb[t][l] * 16;   /* the activations: inputs of l > 0 */
            h->plain_w[slot] = n_plain;
            n_plain += (size_t)o * in;
            h->plain_b[slot] = n_plain;
            n_plain += (size_t)o;
        }
    }
    a.ls_off = (int32_t)off;
    off += 8;
    h->plain_ls = n_plain;
    n_plain += 8;
    a.SX = a.nkb[PI][0] * 16 + 4;
    a.S = widest + 4;
    const size_t n_params = off;
    /* 32 envs per workgroup from 4096 envs on, as the Actor (each workgroup streams every weight
     * once), where the three regions fit */
    h->mt = cfg->n_envs >= 4096 ? 2 : 1;
    if (const char* t = std::getenv("PGX_AC_TILE")) h->mt = std::atoi(t) == 32 ? 2 : 1;
    if (lds_need(a, h->mt) > LDS_LIMIT) h->mt = 1;
    h->lds_bytes = lds_need(a, h->mt);
    if (h->lds_bytes > LDS_LIMIT) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_ac_create: obs_dim too wide for the features in LDS");
    }
    if (hipSetDevice(device) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_ac_create: hipSetDevice");
    }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_plain = al(n_params * 4), o_words = al(o_plain + n_plain * 4), total = o_words + 256;
    if (hipMalloc(&h->blob, total) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_NOMEM, "pgx_ac_create: hipMalloc failed");
    }
    const void* fwd = h->mt == 2 ? (const void*)ac_kernel<2, false> : (const void*)ac_kernel<1, false>;
    const void* val = h->mt == 2 ? (const void*)ac_kernel<2, true> : (const void*)ac_kernel<1, true>;
    if (hipMemset(h->blob, 0, total) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipFuncSetAttribute(fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes) != hipSuccess ||
        hipFuncSetAttribute(val, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes) != hipSuccess) {
        (void)hipFree(h->blob);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_ac_create: device setup failed");
    }
    char* b = (char*)h->blob;
    h->params = (float*)b;
    h->plain = (float*)(b + o_plain);
    a.params = h->params;
    a.step = (unsigned long long*)(b + o_words);
    a.ticket = (uint32_t*)(b + o_words + 8);
    *out = h;
    return PGX_OK;
}

void pgx_ac_destroy(pgx_ac_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->blob);
    delete h;
}

int pgx_ac_set_weights(pgx_ac_handle h, const pgx_ac_weights* w, void* stream) {
    if (!h || !w) return pgx_set_error(PGX_E_INVALID, "pgx_ac_set_weights: null handle or weights");
    const float* W[2][MAX_LINEAR];
    const float* B[2][MAX_LINEAR];
    for (int t = 0; t < 2; t++) {
        const int nl = h->a.n_linear[t] - 1;
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
    for (int t = 0; t < 2; t++)
        for (int l = 0; l < h->a.n_linear[t]; l++, slot++) {
            int o, in;
            linear_dims(h->cfg, t, l, &o, &in);
            /* device parameters are packed where they lie: launches only.  Host ones pass through the
             * handle's staging copy first */
            const float* pw = W[t][l];
            const float* pb = B[t][l];
            if (!on_device(pw) || !on_device(pb)) {
                float* sw = h->plain + h->plain_w[slot];
                float* sb = h->plain + h->plain_b[slot];
                if (hipMemcpyAsync(sw, pw, (size_t)o * in * 4, hipMemcpyDefault, st) != hipSuccess ||
                    hipMemcpyAsync(sb, pb, (size_t)o * 4, hipMemcpyDefault, st) != hipSuccess)
                    return pgx_set_error(PGX_E_HIP, "pgx_ac_set_weights: copy failed");
                pw = sw;
                pb = sb;
            }
            const int n = o * in + o;
            hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pw, pb, h->params + h->a.woff[t][l],
                               h->params + h->a.boff[t][l], o, in, h->a.ntiles[t][l], 0);
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
    launch<false>(h, *io, nullptr, deterministic, (hipStream_t)stream);
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
    launch<true>(h, io, need, 1, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_ac_values: launch failed");
}

int pgx_ac_state(pgx_ac_handle h, uint64_t* step, void* stream) {
    if (!h || !step) return pgx_set_error(PGX_E_INVALID, "pgx_ac_state: null handle or step pointer");
    unsigned long long v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(&v, h->a.step, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_ac_state: device read failed");
    *step = v;
    return PGX_OK;
}

int pgx_ac_set_state(pgx_ac_handle h, uint64_t step, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_ac_set_state: null handle");
    const unsigned long long v = step;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(h->a.step, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_ac_set_state: device write failed");
    return PGX_OK;
}

}  // extern "C"
