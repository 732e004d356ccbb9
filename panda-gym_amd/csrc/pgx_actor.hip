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
 * The noise step word: thread 0 reads it into LDS ahead of the first barrier; the last workgroup
 * to take a ticket, behind every workgroup's read, adds one and clears the ticket.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "../../include/pgx.h"
#include "pgx_common.h"
#include "pgx_mlp.h"   /* linear_layer, pack_kernel, WAVES, NACC, f32x4 */

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */
int pgx_actor_check_config(const pgx_actor_config* c, const char* what, bool with_envs);  /* pgx_actor_host.cpp */

namespace {

constexpr uint32_t TAG_ACTOR = 0x41435430u;
constexpr int THREADS = 64 * WAVES;
constexpr int MAX_LINEAR = PGX_ACTOR_MAX_LAYERS + 1;   /* the hidden layers and the head tile */
constexpr int LOG_STD_ROW = 8;  /* the head tile: mu in rows 0..6, log_std in rows 8..14 */

struct ActorArgs {
    int32_t n, od, ad, n_linear, kind, S;   /* S: LDS row stride (floats) */
    float clip, noise_mu, noise_sigma;
    uint32_t seed_lo, seed_hi;
    int32_t nkb[MAX_LINEAR], ntiles[MAX_LINEAR];   /* 16-wide k blocks and output tiles per Linear */
    int32_t woff[MAX_LINEAR], boff[MAX_LINEAR];    /* packed weights / padded bias, floats into params */
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
    if (tid == 0) sh_step = draw ? *a.step : 0ull;
    /* features: achieved_goal | desired_goal | observation, +0 past in_dim and past env N */
    const int K0 = a.nkb[0] * 16, in_dim = od + 6;
    for (int idx = tid; idx < ROWS * K0; idx += THREADS) {
        const int r = idx / K0, k = idx - r * K0;
        const int e = env0 + r;
        float v = 0.0f;
        if (e < N && k < in_dim) {
            if (k < 3) v = io.achieved_goal[(size_t)e * 3 + k];
            else if (k < 6) v = io.desired_goal[(size_t)e * 3 + (k - 3)];
            else v = io.obs[(size_t)e * od + (k - 6)];
        }
        lds[r * S + k] = v;
    }
    __syncthreads();
    int in_off = 0, out_off = ROWS * S;
    for (int l = 0; l < a.n_linear; l++) {
        linear_layer<MT>(lds, in_off, out_off, a.params + a.woff[l], a.params + a.boff[l], a.nkb[l], a.ntiles[l], S,
                         l + 1 < a.n_linear, lane, wave);
        __syncthreads();
        const int t = in_off;
        in_off = out_off;
        out_off = t;
    }
    /* epilogue: one thread per (env, dimension); the head tile lies at lds[in_off] */
    const int r = tid >> 3, d = tid & 7;
    const int e = env0 + r;
    if (r < ROWS && d < A && e < N) {
        const float* head = lds + in_off + r * S;
        float mean = head[d];
        if (a.clip > 0.0f) mean = mean < -a.clip ? -a.clip : (mean > a.clip ? a.clip : mean);
        float eps = 0.0f;
        if (deterministic == 0) {
            if (io.eps) {
                eps = io.eps[(size_t)e * A + d];
            } else {
                const unsigned long long step = sh_step;
                uint32_t rr[4];
                philox((uint32_t)step, (uint32_t)(step >> 32), (uint32_t)e, TAG_ACTOR ^ (uint32_t)(d >> 1), a.seed_lo,
                       a.seed_hi, rr);
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

}  // namespace

struct pgx_actor {
    int device;
    pgx_actor_config cfg;
    ActorArgs a;
    void* blob;
    float* params;              /* packed weights and padded biases */
    float* plain;               /* the parameters as given, torch layout */
    size_t plain_w[5], plain_b[5];
    int mt;                     /* env tiles of 16 per workgroup */
    size_t lds_bytes;
};

namespace {

constexpr size_t LDS_LIMIT = 160 * 1024;

/* (out, in) of parameter slot i: the hidden layers, mu, log_std */
void slot_dims(const pgx_actor_config& c, int i, int* out, int* in) {
    const int nl = c.n_layers;
    if (i < nl) {
        *out = c.hidden[i];
        *in = i == 0 ? c.obs_dim + 6 : c.hidden[i - 1];
    } else {
        *out = c.action_dim;
        *in = c.hidden[nl - 1];
    }
}

}  // namespace

extern "C" {

int pgx_actor_create(const pgx_actor_config* cfg, int device, pgx_actor_handle* out) {
    const int rc = pgx_actor_check_config(cfg, "pgx_actor_create", true);
    if (rc != PGX_OK) return rc;
    if (!out) return pgx_set_error(PGX_E_INVALID, "pgx_actor_create: null handle pointer");
    *out = nullptr;
    pgx_actor* h = new pgx_actor();
    h->device = device;
    h->cfg = *cfg;
    ActorArgs& a = h->a;
    const int nl = cfg->n_layers, heads = cfg->kind == PGX_ACTOR_GAUSSIAN ? 2 : 1;
    a.n = cfg->n_envs;
    a.od = cfg->obs_dim;
    a.ad = cfg->action_dim;
    a.n_linear = nl + 1;
    a.kind = cfg->kind;
    a.clip = (float)cfg->clip_mean;
    a.noise_mu = (float)cfg->noise_mu;
    a.noise_sigma = (float)cfg->noise_sigma;
    a.seed_lo = (uint32_t)cfg->seed;
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    size_t off = 0;
    int widest = 16;
    for (int l = 0; l <= nl; l++) {
        int o, in;
        slot_dims(*cfg, l, &o, &in);
        a.nkb[l] = (in + 15) / 16;
        a.ntiles[l] = l < nl ? (o + 15) / 16 : 1;
        a.woff[l] = (int32_t)off;
        off += (size_t)a.nkb[l] * a.ntiles[l] * 256;
        a.boff[l] = (int32_t)off;
        off += (size_t)a.ntiles[l] * 16;
        if (a.nkb[l] * 16 > widest) widest = a.nkb[l] * 16;
    }
    a.S = widest + 4;
    const size_t n_params = off;
    size_t n_plain = 0;
    for (int i = 0; i < nl + heads; i++) {
        int o, in;
        slot_dims(*cfg, i, &o, &in);
        h->plain_w[i] = n_plain;
        n_plain += (size_t)o * in;
        h->plain_b[i] = n_plain;
        n_plain += (size_t)o;
    }
    /* 32 envs per workgroup from 4096 envs on: each workgroup streams every weight once, and at
     * 4096 x [256, 256] the halved L2 traffic outweighs the halved workgroup count */
    h->mt = cfg->n_envs >= 4096 ? 2 : 1;
    if (const char* t = std::getenv("PGX_ACTOR_TILE")) h->mt = std::atoi(t) == 32 ? 2 : 1;
    if (2 * (size_t)h->mt * 16 * a.S * 4 > LDS_LIMIT) h->mt = 1;
    h->lds_bytes = 2 * (size_t)h->mt * 16 * a.S * 4;
    if (h->lds_bytes > LDS_LIMIT) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_actor_create: obs_dim too wide for the activations in LDS");
    }
    if (hipSetDevice(device) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_actor_create: hipSetDevice");
    }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_plain = al(n_params * 4), o_words = al(o_plain + n_plain * 4), total = o_words + 256;
    if (hipMalloc(&h->blob, total) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_NOMEM, "pgx_actor_create: hipMalloc failed");
    }
    const void* fn = h->mt == 2 ? (const void*)actor_forward_kernel<2> : (const void*)actor_forward_kernel<1>;
    if (hipMemset(h->blob, 0, total) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes) != hipSuccess) {
        (void)hipFree(h->blob);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_actor_create: device setup failed");
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

void pgx_actor_destroy(pgx_actor_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->blob);
    delete h;
}

int pgx_actor_set_weights(pgx_actor_handle h, const pgx_actor_weights* w, void* stream) {
    if (!h || !w) return pgx_set_error(PGX_E_INVALID, "pgx_actor_set_weights: null handle or weights");
    const int nl = h->cfg.n_layers, heads = h->cfg.kind == PGX_ACTOR_GAUSSIAN ? 2 : 1;
    for (int i = 0; i < nl + heads; i++)
        if (!w->weight[i] || !w->bias[i])
            return pgx_set_error(PGX_E_INVALID, "pgx_actor_set_weights: null weight or bias pointer");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < nl + heads; i++) {
        int o, in;
        slot_dims(h->cfg, i, &o, &in);
        float* pw = h->plain + h->plain_w[i];
        float* pb = h->plain + h->plain_b[i];
        if (hipMemcpyAsync(pw, w->weight[i], (size_t)o * in * 4, hipMemcpyDefault, st) != hipSuccess ||
            hipMemcpyAsync(pb, w->bias[i], (size_t)o * 4, hipMemcpyDefault, st) != hipSuccess)
            return pgx_set_error(PGX_E_HIP, "pgx_actor_set_weights: copy failed");
        const int l = i < nl ? i : nl;
        const int n = o * in + o;
        hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pw, pb, h->params + h->a.woff[l],
                           h->params + h->a.boff[l], o, in, h->a.ntiles[l], i > nl ? LOG_STD_ROW : 0);
    }
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_actor_set_weights: launch failed");
}

int pgx_actor_forward(pgx_actor_handle h, const pgx_actor_io* io, int32_t deterministic, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_actor_forward: null handle or io");
    if (!io->obs || !io->achieved_goal || !io->desired_goal || !io->action)
        return pgx_set_error(PGX_E_INVALID, "pgx_actor_forward: null observation or action pointer");
    const int rows = h->mt * 16;
    const dim3 grid((h->a.n + rows - 1) / rows);
    if (h->mt == 2)
        hipLaunchKernelGGL(actor_forward_kernel<2>, grid, dim3(THREADS), h->lds_bytes, (hipStream_t)stream, h->a, *io,
                           deterministic);
    else
        hipLaunchKernelGGL(actor_forward_kernel<1>, grid, dim3(THREADS), h->lds_bytes, (hipStream_t)stream, h->a, *io,
                           deterministic);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_actor_forward: launch failed");
}

int pgx_actor_state(pgx_actor_handle h, uint64_t* step, void* stream) {
    if (!h || !step) return pgx_set_error(PGX_E_INVALID, "pgx_actor_state: null handle or step pointer");
    unsigned long long v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(&v, h->a.step, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_actor_state: device read failed");
    *step = v;
    return PGX_OK;
}

int pgx_actor_set_state(pgx_actor_handle h, uint64_t step, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_actor_set_state: null handle");
    const unsigned long long v = step;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(h->a.step, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_actor_set_state: device write failed");
    return PGX_OK;
}

}  // extern "C"
