/*
 * pgx_sde_actor.hip -- stable-baselines3's gSDE actor forward for gfx950 (sac/policies.py Actor with
 * use_sde=True, the exploration the reference's TQC trains with: hyperparameters.py), and the
 * resampling of its per-env exploration matrices.  Contract, the matrix draw and the storage layout:
 * include/pgx.h, section "SdeActor".
 *
 * Forward kernel: the Actor's workgroup (pgx_actor.hip) -- 4 waves own a tile of 16 (or 32) envs,
 * activations stay in LDS, every Linear is pgx_mlp.h's MFMA chain.  After the last trunk layer the
 * latent lies in LDS; wave 0 runs the mu head tile while the lanes that own an (env, a) pair, dealt
 * from wave 3 downwards, run the noise chain: H dependent fmaf on the latent (one 16-byte LDS read
 * per four h) against the env's matrix, streamed from global memory as one 16-byte load per lane per
 * four h, PF loads in flight ahead of the chain.  The storage layout S[e / 16][h / 4][e % 16][a][h % 4]
 * makes the loads of the lanes of 16 envs one contiguous run of 256 A bytes per h block.  Behind the
 * barrier the same lanes read their mean from the head tile and finish the action.
 *
 * Reset kernel: thread g of the grid owns the 16 bytes g of the storage, i.e. (tile, h block, env,
 * i < A) -- and draws block q = (h block) A + i of that env, whose four flat indices 4 q .. 4 q + 3
 * are, transposed, exactly the 4 A floats of that env's h block.  The A lanes of one (env, h block)
 * exchange them through LDS, so every lane stores the one contiguous 16 bytes it owns.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "../../include/pgx.h"
#include "pgx_common.h"
#include "pgx_mlp.h"   /* linear_layer, pack_kernel, WAVES, NACC, f32x4 */

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */
int pgx_sde_actor_check_config(const pgx_sde_actor_config* c, const char* what, bool with_envs);  /* pgx_actor_host.cpp */

namespace {

constexpr int THREADS = 64 * WAVES;
constexpr int MAX_LINEAR = PGX_ACTOR_MAX_LAYERS + 1;   /* the hidden layers and the mu tile */
constexpr int PF = 4;                                  /* 16-byte matrix loads in flight per lane */

struct SdeArgs {
    int32_t n, od, ad, n_linear, S, H, H4;   /* S: LDS row stride (floats); H4: h blocks of 4 */
    float clip;
    uint32_t seed_lo, seed_hi;
    int32_t nkb[MAX_LINEAR], ntiles[MAX_LINEAR];   /* 16-wide k blocks and output tiles per Linear */
    int32_t woff[MAX_LINEAR], boff[MAX_LINEAR];    /* packed weights / padded bias, floats into params */
    const float* params;
    float* E;                  /* the matrices, storage layout */
    float* std;                /* [H, A] */
    unsigned long long* gen;
    uint32_t* ticket;
};

/* the epilogue, every operation rounded on its own */
__device__ __forceinline__ float squash(float mean, float noise, bool deterministic) {
#pragma clang fp contract(off)
    return tanhf(deterministic ? mean : mean + noise);
}

template <int MT>
__global__ __launch_bounds__(THREADS) void sde_forward_kernel(SdeArgs a, pgx_sde_actor_io io, int32_t deterministic) {
    extern __shared__ float lds[];
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, N = a.n, od = a.od, A = a.ad, H = a.H;
    const int env0 = blockIdx.x * ROWS;
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
    for (int l = 0; l + 1 < a.n_linear; l++) {
        linear_layer<MT>(lds, in_off, out_off, a.params + a.woff[l], a.params + a.boff[l], a.nkb[l], a.ntiles[l], S, true,
                         lane, wave);
        __syncthreads();
        const int t = in_off;
        in_off = out_off;
        out_off = t;
    }
    /* the latent lies at lds[in_off]; the mu tile goes to lds[out_off] (one tile: wave 0) */
    const int lm = a.n_linear - 1;
    linear_layer<MT>(lds, in_off, out_off, a.params + a.woff[lm], a.params + a.boff[lm], a.nkb[lm], 1, S, false, lane, wave);
    /* the noise chain: pair p = r A + a, dealt from wave 3 downwards */
    const int p = (WAVES - 1 - wave) * 64 + lane;
    const int r = p / A, d = p - r * A;
    const int e = env0 + r;
    const bool own = r < ROWS && e < N;
    float noise = 0.0f;
    if (own && deterministic == 0) {
        const float* lat = lds + in_off + r * S;
        const int H4 = a.H4, Hfull = H >> 2;
        /* f32x4 g of the storage: ((e / 16) H4 + hb) 16 A + (e % 16) A + a */
        const f32x4* Ev = reinterpret_cast<const f32x4*>(a.E) + (size_t)(e >> 4) * H4 * 16 * A + (e & 15) * A + d;
        const int hstride = 16 * A;
        const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
        f32x4 cur[PF], nxt[PF];
#pragma unroll
        for (int i = 0; i < PF; i++) cur[i] = i < H4 ? Ev[(size_t)i * hstride] : zero4;
        float acc = 0.0f;
        const int rem = H & 3;   /* terms of the last h block where H is no multiple of 4 */
        for (int hb0 = 0; hb0 < H4; hb0 += PF) {
#pragma unroll
            for (int i = 0; i < PF; i++) nxt[i] = hb0 + PF + i < H4 ? Ev[(size_t)(hb0 + PF + i) * hstride] : zero4;
#pragma unroll
            for (int i = 0; i < PF; i++) {
                const int hb = hb0 + i;
                if (hb >= H4) break;
                const f32x4 l4 = *reinterpret_cast<const f32x4*>(lat + 4 * hb);
                acc = __builtin_fmaf(l4[0], cur[i][0], acc);
                if (hb < Hfull || rem > 1) acc = __builtin_fmaf(l4[1], cur[i][1], acc);
                if (hb < Hfull || rem > 2) acc = __builtin_fmaf(l4[2], cur[i][2], acc);
                if (hb < Hfull) acc = __builtin_fmaf(l4[3], cur[i][3], acc);
            }
#pragma unroll
            for (int i = 0; i < PF; i++) cur[i] = nxt[i];
        }
        noise = acc;
    }
    __syncthreads();
    if (own) {
        float mean = lds[out_off + r * S + d];
        if (a.clip > 0.0f) mean = mean < -a.clip ? -a.clip : (mean > a.clip ? a.clip : mean);
        io.action[(size_t)e * A + d] = squash(mean, noise, deterministic != 0);
        if (io.mean_out) io.mean_out[(size_t)e * A + d] = mean;
        if (io.noise_out) io.noise_out[(size_t)e * A + d] = noise;
    }
    if (io.latent_out)
        for (int idx = tid; idx < ROWS * H; idx += THREADS) {
            const int rr = idx / H, h = idx - rr * H;
            if (env0 + rr < N) io.latent_out[(size_t)(env0 + rr) * H + h] = lds[in_off + rr * S + h];
        }
}

/* blockDim.x = 16 A KB: KB whole h blocks of one tile of 16 envs; grid (ceil(H4 / KB), tiles) */
__global__ __launch_bounds__(THREADS) void sde_reset_kernel(SdeArgs a, int KB, float* eps_out, uint32_t* philox_out) {
    __shared__ float sh[THREADS * 4];
    __shared__ unsigned long long sh_gen;
    const int tid = threadIdx.x, A = a.ad, H = a.H, H4 = a.H4;
    if (tid == 0) sh_gen = *a.gen;
    __syncthreads();
    const int i = tid % A, r = (tid / A) & 15, hbl = tid / (16 * A);
    const int hb = blockIdx.x * KB + hbl, tile = blockIdx.y;
    const int e = tile * 16 + r;
    const int q = hb * A + i;
    const bool live = hb < H4 && e < a.n;
    if (live) {
        const unsigned long long gen = sh_gen;
        uint32_t rr[4];
        philox((uint32_t)gen, (uint32_t)(gen >> 32), (uint32_t)e, PGX_SDE_PHILOX_TAG ^ (uint32_t)q, a.seed_lo, a.seed_hi, rr);
        float eps[4];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float u1 = (float)((rr[2 * c] >> 8) + 1u) * 5.9604644775390625e-8f;
            const float u2 = (float)(rr[2 * c + 1] >> 8) * 5.9604644775390625e-8f;
            const float rad = sqrtf(-2.0f * logf(u1)), ang = 6.2831855f * u2;
            eps[2 * c] = rad * cosf(ang);
            eps[2 * c + 1] = rad * sinf(ang);
        }
        if (philox_out && q < 4) {
            uint32_t* o = philox_out + ((size_t)e * 4 + q) * 4;
            o[0] = rr[0]; o[1] = rr[1]; o[2] = rr[2]; o[3] = rr[3];
        }
        float* chunk = sh + (tid - i) * 4;   /* the 4 A floats of (env, h block): [a][h % 4] */
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int jl = 4 * i + c;            /* flat index inside the h block: (h % 4) A + a */
            const int hl = jl / A, d = jl - hl * A;
            const int h = 4 * hb + hl;
            float v = 0.0f;                      /* past H: the padding stays +0 */
            if (h < H) {
                const int j = h * A + d;
                v = eps[c] * a.std[j];
                if (eps_out) eps_out[(size_t)e * H * A + j] = eps[c];
            }
            chunk[d * 4 + hl] = v;
        }
    }
    __syncthreads();
    if (live) {
        const size_t g = ((size_t)tile * H4 + hb) * 16 * A + r * A + i;
        reinterpret_cast<f32x4*>(a.E)[g] = *reinterpret_cast<const f32x4*>(sh + tid * 4);
    }
    /* every workgroup has read the generation word (ahead of its first barrier): the last one to
     * arrive moves it on */
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(a.ticket, 1u) == gridDim.x * gridDim.y - 1) {
            *a.ticket = 0u;
            *a.gen = sh_gen + 1ull;
        }
    }
}

/* SB3's [N, H, A] <-> the storage layout, one thread per element */
__global__ __launch_bounds__(256) void sde_translate_kernel(SdeArgs a, float* plain, const float* src, int to_storage) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t HA = (size_t)a.H * a.ad;
    if (idx >= (size_t)a.n * HA) return;
    const int e = (int)(idx / HA), j = (int)(idx - (size_t)e * HA);
    const int h = j / a.ad, d = j - h * a.ad;
    const size_t s = ((((size_t)(e >> 4) * a.H4 + (h >> 2)) * 16 + (e & 15)) * a.ad + d) * 4 + (h & 3);
    if (to_storage) a.E[s] = src[idx];
    else plain[idx] = a.E[s];
}

/* std = expf(log_std), or (out != NULL) a copy of std */
__global__ __launch_bounds__(256) void sde_std_kernel(const float* log_std, float* std, float* out, int n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    if (out) out[idx] = std[idx];
    else std[idx] = expf(log_std[idx]);
}

}  // namespace

struct pgx_sde_actor {
    int device;
    pgx_sde_actor_config cfg;
    SdeArgs a;
    void* blob;
    float* params;              /* packed weights and padded biases */
    float* plain;               /* the parameters as given, torch layout; log_std last */
    size_t plain_w[4], plain_b[4], plain_ls;
    int mt;                     /* env tiles of 16 per workgroup */
    int kb;                     /* h blocks per reset workgroup */
    size_t lds_bytes;
};

namespace {

constexpr size_t LDS_LIMIT = 160 * 1024;

/* (out, in) of parameter slot i: the hidden layers, mu */
void slot_dims(const pgx_sde_actor_config& c, int i, int* out, int* in) {
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

int pgx_sde_actor_create(const pgx_sde_actor_config* cfg, int device, pgx_sde_actor_handle* out) {
    const int rc = pgx_sde_actor_check_config(cfg, "pgx_sde_actor_create", true);
    if (rc != PGX_OK) return rc;
    if (!out) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_create: null handle pointer");
    *out = nullptr;
    pgx_sde_actor* h = new pgx_sde_actor();
    h->device = device;
    h->cfg = *cfg;
    SdeArgs& a = h->a;
    const int nl = cfg->n_layers;
    a.n = cfg->n_envs;
    a.od = cfg->obs_dim;
    a.ad = cfg->action_dim;
    a.n_linear = nl + 1;
    a.H = cfg->hidden[nl - 1];
    a.H4 = (a.H + 3) / 4;
    a.clip = (float)cfg->clip_mean;
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
    for (int i = 0; i <= nl; i++) {
        int o, in;
        slot_dims(*cfg, i, &o, &in);
        h->plain_w[i] = n_plain;
        n_plain += (size_t)o * in;
        h->plain_b[i] = n_plain;
        n_plain += (size_t)o;
    }
    h->plain_ls = n_plain;
    const size_t n_std = (size_t)a.H * a.ad;
    n_plain += n_std;
    /* 32 envs per workgroup from 4096 envs on, as the Actor */
    h->mt = cfg->n_envs >= 4096 ? 2 : 1;
    if (2 * (size_t)h->mt * 16 * a.S * 4 > LDS_LIMIT) h->mt = 1;
    h->lds_bytes = 2 * (size_t)h->mt * 16 * a.S * 4;
    if (h->lds_bytes > LDS_LIMIT) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_sde_actor_create: obs_dim too wide for the activations in LDS");
    }
    h->kb = THREADS / (16 * a.ad);
    if (hipSetDevice(device) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_create: hipSetDevice");
    }
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t tiles = ((size_t)cfg->n_envs + 15) / 16;
    const size_t n_E = tiles * a.H4 * 16 * a.ad * 4;
    const size_t o_plain = al(n_params * 4), o_std = al(o_plain + n_plain * 4), o_E = al(o_std + n_std * 4),
                 o_words = al(o_E + n_E * 4), total = o_words + 256;
    if (hipMalloc(&h->blob, total) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_NOMEM, "pgx_sde_actor_create: hipMalloc failed");
    }
    const void* fn = h->mt == 2 ? (const void*)sde_forward_kernel<2> : (const void*)sde_forward_kernel<1>;
    if (hipMemset(h->blob, 0, total) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes) != hipSuccess) {
        (void)hipFree(h->blob);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_create: device setup failed");
    }
    char* b = (char*)h->blob;
    h->params = (float*)b;
    h->plain = (float*)(b + o_plain);
    a.params = h->params;
    a.std = (float*)(b + o_std);
    a.E = (float*)(b + o_E);
    a.gen = (unsigned long long*)(b + o_words);
    a.ticket = (uint32_t*)(b + o_words + 8);
    *out = h;
    return PGX_OK;
}

void pgx_sde_actor_destroy(pgx_sde_actor_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->blob);
    delete h;
}

int pgx_sde_actor_set_weights(pgx_sde_actor_handle h, const pgx_sde_actor_weights* w, void* stream) {
    if (!h || !w) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_set_weights: null handle or weights");
    const int nl = h->cfg.n_layers;
    for (int i = 0; i <= nl; i++)
        if (!w->weight[i] || !w->bias[i])
            return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_set_weights: null weight or bias pointer");
    if (!w->log_std) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_set_weights: null log_std pointer");
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i <= nl; i++) {
        int o, in;
        slot_dims(h->cfg, i, &o, &in);
        float* pw = h->plain + h->plain_w[i];
        float* pb = h->plain + h->plain_b[i];
        if (hipMemcpyAsync(pw, w->weight[i], (size_t)o * in * 4, hipMemcpyDefault, st) != hipSuccess ||
            hipMemcpyAsync(pb, w->bias[i], (size_t)o * 4, hipMemcpyDefault, st) != hipSuccess)
            return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_weights: copy failed");
        const int n = o * in + o;
        hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pw, pb, h->params + h->a.woff[i],
                           h->params + h->a.boff[i], o, in, h->a.ntiles[i], 0);
    }
    const int n_std = h->a.H * h->a.ad;
    float* ls = h->plain + h->plain_ls;
    if (hipMemcpyAsync(ls, w->log_std, (size_t)n_std * 4, hipMemcpyDefault, st) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_weights: copy failed");
    hipLaunchKernelGGL(sde_std_kernel, dim3((n_std + 255) / 256), dim3(256), 0, st, (const float*)ls, h->a.std,
                       (float*)nullptr, n_std);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_weights: launch failed");
}

int pgx_sde_actor_reset_noise(pgx_sde_actor_handle h, float* eps_out, uint32_t* philox_out, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_reset_noise: null handle");
    const int kb = h->kb;
    const dim3 grid((h->a.H4 + kb - 1) / kb, (h->a.n + 15) / 16);
    hipLaunchKernelGGL(sde_reset_kernel, grid, dim3(16 * h->a.ad * kb), 0, (hipStream_t)stream, h->a, kb, eps_out, philox_out);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_reset_noise: launch failed");
}

int pgx_sde_actor_forward(pgx_sde_actor_handle h, const pgx_sde_actor_io* io, int32_t deterministic, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_forward: null handle or io");
    if (!io->obs || !io->achieved_goal || !io->desired_goal || !io->action)
        return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_forward: null observation or action pointer");
    const int rows = h->mt * 16;
    const dim3 grid((h->a.n + rows - 1) / rows);
    if (h->mt == 2)
        hipLaunchKernelGGL(sde_forward_kernel<2>, grid, dim3(THREADS), h->lds_bytes, (hipStream_t)stream, h->a, *io,
                           deterministic);
    else
        hipLaunchKernelGGL(sde_forward_kernel<1>, grid, dim3(THREADS), h->lds_bytes, (hipStream_t)stream, h->a, *io,
                           deterministic);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_forward: launch failed");
}

int pgx_sde_actor_state(pgx_sde_actor_handle h, uint64_t* generation, void* stream) {
    if (!h || !generation) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_state: null handle or generation pointer");
    unsigned long long v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(&v, h->a.gen, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_state: device read failed");
    *generation = v;
    return PGX_OK;
}

int pgx_sde_actor_set_state(pgx_sde_actor_handle h, uint64_t generation, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_set_state: null handle");
    const unsigned long long v = generation;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(h->a.gen, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_state: device write failed");
    return PGX_OK;
}

int pgx_sde_actor_get_matrices(pgx_sde_actor_handle h, float* out, void* stream) {
    if (!h || !out) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_get_matrices: null handle or out pointer");
    const size_t n = (size_t)h->a.n * h->a.H * h->a.ad;
    hipLaunchKernelGGL(sde_translate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->a, out,
                       (const float*)nullptr, 0);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_get_matrices: launch failed");
}

int pgx_sde_actor_set_matrices(pgx_sde_actor_handle h, const float* in, void* stream) {
    if (!h || !in) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_set_matrices: null handle or in pointer");
    const size_t n = (size_t)h->a.n * h->a.H * h->a.ad;
    hipLaunchKernelGGL(sde_translate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->a,
                       (float*)nullptr, in, 1);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_matrices: launch failed");
}

int pgx_sde_actor_get_std(pgx_sde_actor_handle h, float* out, void* stream) {
    if (!h || !out) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_get_std: null handle or out pointer");
    const int n_std = h->a.H * h->a.ad;
    hipLaunchKernelGGL(sde_std_kernel, dim3((n_std + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)nullptr,
                       h->a.std, out, n_std);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_get_std: launch failed");
}

}  // extern "C"
