/*
 * pgx_sde_actor.hip -- stable-baselines3's gSDE actor forward for gfx950 (sac/policies.py Actor with
 * use_sde=True, the exploration the reference's TQC trains with: hyperparameters.py), and the
 * resampling of its per-env exploration matrices.  Contract, the matrix draw and the storage layout:
 * include/pgx.h, section "SdeActor".
 *
 * Forward kernel: the Actor's workgroup (pgx_actor.hip) -- 4 waves own a tile of 16 (or 32) envs,
 * activations stay in LDS; the staging, the Linear and the loop over the trunk's layers are pgx_mlp.h's,
 * the host-side plan, allocation and packing pgx_policy.h's.  After the last trunk layer the
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
 *
 * Log-probability kernel (pgx_sde_actor_action_log_prob, SB3's actor.action_log_prob as TQC.train reaches
 * it): the forward's workgroup over a tile of 32 batch rows (16 for a batch of up to 16, or where 32 do
 * not fit the LDS), read through their row strides.  The noise of a batch comes from ONE shared matrix Eb
 * [H, A], kept plain and packed into rows 8..14 of mu's tile, so the head tile's MFMAs give mean and noise
 * together; the latent is then squared in place and a second tile, std2 = std * std packed at
 * set_weights, gives the variance over the squares.  The epilogue (the inverse of the squash, the Gaussian
 * density, the correction) runs with contraction off, one thread per (row, dimension), and the sums go
 * through the dead activations.  pgx_sde_actor_reset_batch_noise draws Eb with a generation word and a
 * counter tag of its own; the per-env matrices never see any of this.
 */
#include "pgx_policy.h"   /* pgx_mlp.h, pgx_common.h, include/pgx.h */

/* pgx_actor_host.cpp */
int pgx_sde_actor_check_config(const pgx_sde_actor_config* c, const char* what, bool with_envs);
int pgx_sde_actor_lp_check_launch(const pgx_sde_actor_config* c, const pgx_sde_actor_lp_io* io, int32_t B, const char* what);

namespace {

constexpr int PF = 4;                                  /* 16-byte matrix loads in flight per lane */

struct SdeArgs {
    int32_t n, od, ad, S, H, H4;   /* S: LDS row stride (floats); H4: h blocks of 4 */
    float clip;
    uint32_t seed_lo, seed_hi;
    MlpPlan plan;                  /* the trunk and the mu tile */
    const float* params;
    float* E;                  /* the matrices, storage layout */
    float* std;                /* [H, A] */
    unsigned long long* gen;
    uint32_t* ticket;
};

/* what the batch entries use beside SdeArgs: the shared matrix Eb and std2, plain [H, A] and packed */
struct SdeBatch {
    float* Eb;                 /* [H, A] */
    float* std2;               /* [H, A] */
    float* Pmu;                /* mu's packed tile: Eb goes to its rows 8..14 */
    float* P2;                 /* std2's packed tile (rows 0..6), its 16 bias floats (+0) behind it */
    unsigned long long* gen;
    uint32_t* ticket;
};

/* element (output row, k) of a packed Linear of one tile: pgx_mlp.h's pack_kernel with ntiles = 1 */
__device__ __forceinline__ int packed_index(int row, int k) {
    return (((k >> 4) * 64) + (k & 3) * 16 + row) * 4 + ((k >> 2) & 3);
}

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
    const int S = a.S, N = a.n, od = a.od, A = a.ad;
    const int env0 = blockIdx.x * ROWS;
    stage_features<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, env0, N, od, a.plan.nkb[0] * 16, S, tid);
    __syncthreads();
    /* the trunk, every layer with its ReLU: the features lie in region 0; it and region ROWS * S take turns */
    const int lm = a.plan.n_linear - 1;
    const int in_off = run_linears<MT>(lds, a.params, a.plan, lm, true, 0, S, ROWS * S, 0, S, lane, wave);
    const int out_off = in_off == 0 ? ROWS * S : 0;
    /* the latent lies at lds[in_off]; the mu tile goes to lds[out_off] (one tile: wave 0), and no barrier
     * stands between it and the noise chain */
    linear_layer<MT>(lds, in_off, out_off, a.params + a.plan.woff[lm], a.params + a.plan.boff[lm], a.plan.nkb[lm], 1, S,
                     false, lane, wave);
    /* the noise chain: pair p = r A + a, dealt from wave 3 downwards */
    const int H = a.H;
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

/* the log-probability epilogue of one (row, dimension), every operation rounded on its own */
__device__ __forceinline__ void sde_lp_terms(float mean, float noise, float var, float* act, float* gp, float* lp, float* c) {
#pragma clang fp contract(off)
    const float scale = sqrtf(var + 1e-6f);
    const float a = tanhf(mean + noise);
    const float lim = 1.0f - 1.1920929e-7f;
    const float x = a < -lim ? -lim : (a > lim ? lim : a);
    const float g = 0.5f * (log1pf(x) - log1pf(-x));
    const float z = g - mean;
    *lp = ((-(z * z)) / (2.0f * (scale * scale)) - logf(scale)) - 0.9189385f;
    const float t = tanhf(g);
    *c = logf((1.0f - t * t) + 1e-6f);
    *act = a;
    *gp = g;
}

/* pgx_sde_actor_action_log_prob: the forward's workgroup over a tile of batch rows read through their
 * strides (a.n is the batch size).  Behind the trunk the head tile gives mean (rows 0..6) and the noise
 * chain against Eb (rows 8..14); their owners take them into registers, the latent is squared in place,
 * and std2's tile over the squares gives the variance where the head tile lay. */
template <int MT>
__global__ __launch_bounds__(THREADS) void sde_lp_kernel(SdeArgs a, SdeBatch bt, pgx_sde_actor_lp_io io) {
    extern __shared__ float lds[];
    constexpr int ROWS = MT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, B = a.n, A = a.ad, H = a.H;
    const int row0 = blockIdx.x * ROWS;
    stage_rows<MT>(lds, io.obs, io.achieved_goal, io.desired_goal, nullptr, io.obs_stride, io.achieved_goal_stride,
                   io.desired_goal_stride, 0, row0, B, a.od, 0, a.plan.nkb[0] * 16, S, tid);
    __syncthreads();
    const int lm = a.plan.n_linear - 1;
    const int in_off = run_linears<MT>(lds, a.params, a.plan, lm, true, 0, S, ROWS * S, 0, S, lane, wave);
    const int out_off = in_off == 0 ? ROWS * S : 0;
    const int nkb = a.plan.nkb[lm];
    linear_layer<MT>(lds, in_off, out_off, a.params + a.plan.woff[lm], a.params + a.plan.boff[lm], nkb, 1, S, false, lane,
                     wave);
    __syncthreads();
    const int r = tid >> 3, d = tid & 7;
    const int b = row0 + r;
    const bool own = r < ROWS && d < A && b < B;
    float mean = 0.0f, noise = 0.0f;
    if (own) {
        mean = lds[out_off + r * S + d];
        if (a.clip > 0.0f) mean = mean < -a.clip ? -a.clip : (mean > a.clip ? a.clip : mean);
        noise = lds[out_off + r * S + 8 + d];
    }
    const int K16 = nkb * 16;
    for (int idx = tid; idx < ROWS * K16; idx += THREADS) {
        const int rr = idx / K16, h = idx - rr * K16;
        const float v = lds[in_off + rr * S + h];
        if (io.latent_out && h < H && row0 + rr < B) io.latent_out[(size_t)(row0 + rr) * H + h] = v;
        lds[in_off + rr * S + h] = v * v;
    }
    __syncthreads();
    linear_layer<MT>(lds, in_off, out_off, bt.P2, bt.P2 + nkb * 256, nkb, 1, S, false, lane, wave);
    __syncthreads();
    float lp = 0.0f, c = 0.0f;
    if (own) {
        const float var = lds[out_off + r * S + d];
        float act, g;
        sde_lp_terms(mean, noise, var, &act, &g, &lp, &c);
        const size_t o = (size_t)b * A + d;
        io.action[o] = act;
        if (io.mean_out) io.mean_out[o] = mean;
        if (io.noise_out) io.noise_out[o] = noise;
        if (io.variance_out) io.variance_out[o] = var;
        if (io.gaussian_action_out) io.gaussian_action_out[o] = g;
    }
    __syncthreads();   /* the variance tile is read: the activations are dead and carry the sums' terms */
    sum_log_prob(lds, lp, c, own, A, io.log_prob, (size_t)b, tid);
}

/* pgx_sde_actor_reset_batch_noise: thread q of the grid draws block q of the shared matrix, flat indices
 * 4 q .. 4 q + 3, and stores each both plain and where mu's packed tile holds it */
__global__ __launch_bounds__(THREADS) void sde_batch_reset_kernel(SdeArgs a, SdeBatch bt, float* eps_out) {
    __shared__ unsigned long long sh_gen;
    const int tid = threadIdx.x;
    load_word(&sh_gen, bt.gen, true, tid);
    __syncthreads();
    const int q = blockIdx.x * THREADS + tid, HA = a.H * a.ad;
    if (4 * q < HA) {
        const unsigned long long gen = sh_gen;
        uint32_t rr[4];
        philox((uint32_t)gen, (uint32_t)(gen >> 32), 0u, PGX_SDE_BATCH_PHILOX_TAG ^ (uint32_t)q, a.seed_lo, a.seed_hi, rr);
        float eps[4];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            float rad, ang;
            box_muller(rr[2 * c], rr[2 * c + 1], &rad, &ang);
            eps[2 * c] = rad * cosf(ang);
            eps[2 * c + 1] = rad * sinf(ang);
        }
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int j = 4 * q + c;
            if (j >= HA) break;
            const int h = j / a.ad, d = j - h * a.ad;
            const float v = eps[c] * a.std[j];
            bt.Eb[j] = v;
            bt.Pmu[packed_index(8 + d, h)] = v;
            if (eps_out) eps_out[j] = eps[c];
        }
    }
    advance_word(bt.gen, bt.ticket, &sh_gen, gridDim.x, true, tid);
}

/* the shared matrix from SB3's [H, A] (in != NULL: plain and packed), or into it */
__global__ __launch_bounds__(256) void sde_batch_copy_kernel(SdeArgs a, SdeBatch bt, const float* in, float* out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.H * a.ad) return;
    if (in) {
        const int h = j / a.ad, d = j - h * a.ad;
        const float v = in[j];
        bt.Eb[j] = v;
        bt.Pmu[packed_index(8 + d, h)] = v;
    } else {
        out[j] = bt.Eb[j];
    }
}

/* blockDim.x = 16 A KB: KB whole h blocks of one tile of 16 envs; grid (ceil(H4 / KB), tiles) */
__global__ __launch_bounds__(THREADS) void sde_reset_kernel(SdeArgs a, int KB, float* eps_out, uint32_t* philox_out) {
    __shared__ float sh[THREADS * 4];
    __shared__ unsigned long long sh_gen;
    const int tid = threadIdx.x, A = a.ad, H = a.H, H4 = a.H4;
    load_word(&sh_gen, a.gen, true, tid);
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
            float rad, ang;
            box_muller(rr[2 * c], rr[2 * c + 1], &rad, &ang);
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
    advance_word(a.gen, a.ticket, &sh_gen, gridDim.x * gridDim.y, true, tid);
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

/* std = expf(log_std) and std2 = std * std (plain and packed: A the action dimension), or (out != NULL) a
 * copy of std */
__global__ __launch_bounds__(256) void sde_std_kernel(const float* log_std, float* std, float* out, int n, float* std2,
                                                      float* P2, int A) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    if (out) {
        out[idx] = std[idx];
        return;
    }
    const float s = expf(log_std[idx]);
    const float s2 = s * s;
    const int h = idx / A;
    std[idx] = s;
    std2[idx] = s2;
    P2[packed_index(idx - h * A, h)] = s2;
}

}  // namespace

struct pgx_sde_actor {
    int device;
    pgx_sde_actor_config cfg;
    SdeArgs a;
    float* params;              /* packed weights and padded biases; the head of the one allocation */
    float* plain;               /* the parameters as given, torch layout; log_std last */
    size_t plain_w[4], plain_b[4], plain_ls;
    int mt;                     /* env tiles of 16 per workgroup */
    int kb;                     /* h blocks per reset workgroup */
    size_t lds_bytes;
    SdeBatch bt;

    size_t lds_need(int mt) const { return 2 * (size_t)mt * 16 * a.S * 4; }
    /* row tiles of 16 per workgroup of a batch launch: 32 rows from 17 on, where they fit the LDS */
    int lp_tile(int B) const {
        return choose_tile(B, "PGX_SDE_LP_TILE", [this](int mt) { return lds_need(mt); }, 17);
    }
};

extern "C" {

int pgx_sde_actor_create(const pgx_sde_actor_config* cfg, int device, pgx_sde_actor_handle* out) {
    int rc = pgx_sde_actor_check_config(cfg, "pgx_sde_actor_create", true);
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
    a.H = cfg->hidden[nl - 1];
    a.H4 = (a.H + 3) / 4;
    a.clip = (float)cfg->clip_mean;
    a.seed_lo = (uint32_t)cfg->seed;
    a.seed_hi = (uint32_t)(cfg->seed >> 32);
    size_t n_params = 0, n_plain = 0;
    a.S = 4 + plan_stack(&a.plan, cfg->obs_dim + 6, cfg->hidden, nl, cfg->action_dim, 0, &n_params, h->plain_w,
                         h->plain_b, &n_plain);
    h->plain_ls = n_plain;
    const size_t n_std = (size_t)a.H * a.ad;
    n_plain += n_std;
    /* the tile as the Actor chooses it, without an override */
    auto lds_need = [&a](int mt) { return 2 * (size_t)mt * 16 * a.S * 4; };
    h->mt = choose_tile(cfg->n_envs, nullptr, lds_need);
    if (h->mt == 0) {
        delete h;
        return pgx_set_error(PGX_E_UNSUPPORTED, "pgx_sde_actor_create: obs_dim too wide for the activations in LDS");
    }
    h->lds_bytes = lds_need(h->mt);
    h->kb = THREADS / (16 * a.ad);
    const size_t tiles = ((size_t)cfg->n_envs + 15) / 16;
    /* the last region: std2's packed tile and bias, then Eb and std2 plain */
    const size_t n_p2 = (size_t)a.plan.nkb[nl] * 256 + 16;
    const size_t bytes[6] = {n_params * 4, n_plain * 4, n_std * 4, tiles * a.H4 * 16 * a.ad * 4 * 4, 256,
                             (n_p2 + 2 * n_std) * 4};
    void* ptr[6];
    const void* fn = h->mt == 2 ? (const void*)sde_forward_kernel<2> : (const void*)sde_forward_kernel<1>;
    rc = create_blob("pgx_sde_actor_create", device, bytes, 6, ptr, {fn}, h->lds_bytes);
    if (rc != PGX_OK) {
        delete h;
        return rc;
    }
    a.params = h->params = (float*)ptr[0];
    h->plain = (float*)ptr[1];
    a.std = (float*)ptr[2];
    a.E = (float*)ptr[3];
    a.gen = (unsigned long long*)ptr[4];
    a.ticket = (uint32_t*)((char*)ptr[4] + 8);
    h->bt.gen = (unsigned long long*)((char*)ptr[4] + 16);
    h->bt.ticket = (uint32_t*)((char*)ptr[4] + 24);
    h->bt.Pmu = h->params + a.plan.woff[nl];
    h->bt.P2 = (float*)ptr[5];
    h->bt.Eb = h->bt.P2 + n_p2;
    h->bt.std2 = h->bt.Eb + n_std;
    if (!set_tile_lds(sde_lp_kernel<1>, sde_lp_kernel<2>, lds_need)) {
        (void)hipFree(h->params);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_create: device setup failed");
    }
    *out = h;
    return PGX_OK;
}

void pgx_sde_actor_destroy(pgx_sde_actor_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->params);
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
    const MlpPlan& p = h->a.plan;
    for (int i = 0; i <= nl; i++) {
        int o, in;
        linear_dims(h->cfg.obs_dim + 6, h->cfg.hidden, nl, h->cfg.action_dim, i, &o, &in);
        if (!pack_linear(w->weight[i], w->bias[i], h->plain + h->plain_w[i], h->plain + h->plain_b[i], o, in,
                         h->params + p.woff[i], h->params + p.boff[i], p.ntiles[i], 0, st))
            return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_weights: copy failed");
    }
    const int n_std = h->a.H * h->a.ad;
    float* ls = h->plain + h->plain_ls;
    if (hipMemcpyAsync(ls, w->log_std, (size_t)n_std * 4, hipMemcpyDefault, st) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_sde_actor_set_weights: copy failed");
    hipLaunchKernelGGL(sde_std_kernel, dim3((n_std + 255) / 256), dim3(256), 0, st, (const float*)ls, h->a.std,
                       (float*)nullptr, n_std, h->bt.std2, h->bt.P2, h->a.ad);
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
    launch_tiles(sde_forward_kernel<1>, sde_forward_kernel<2>, h->mt, h->a.n, h->lds_bytes, stream, h->a, *io,
                 deterministic);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_forward: launch failed");
}

int pgx_sde_actor_action_log_prob(pgx_sde_actor_handle h, const pgx_sde_actor_lp_io* io, int32_t B, void* stream) {
    const char* what = "pgx_sde_actor_action_log_prob";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int rc = pgx_sde_actor_lp_check_launch(&h->cfg, io, B, what);
    if (rc != PGX_OK) return rc;
    SdeArgs a = h->a;
    a.n = B;
    const int mt = h->lp_tile(B);
    launch_tiles(sde_lp_kernel<1>, sde_lp_kernel<2>, mt, B, h->lds_need(mt), stream, a, h->bt, *io);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_sde_actor_reset_batch_noise(pgx_sde_actor_handle h, float* eps_out, void* stream) {
    const char* what = "pgx_sde_actor_reset_batch_noise";
    if (!h) return fail(PGX_E_INVALID, what, "null handle");
    const int nq = (h->a.H * h->a.ad + 3) / 4;
    hipLaunchKernelGGL(sde_batch_reset_kernel, dim3((nq + THREADS - 1) / THREADS), dim3(THREADS), 0, (hipStream_t)stream,
                       h->a, h->bt, eps_out);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_sde_actor_get_batch_matrix(pgx_sde_actor_handle h, float* out, void* stream) {
    const char* what = "pgx_sde_actor_get_batch_matrix";
    if (!h || !out) return fail(PGX_E_INVALID, what, "null handle or out pointer");
    hipLaunchKernelGGL(sde_batch_copy_kernel, dim3((h->a.H * h->a.ad + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->a,
                       h->bt, (const float*)nullptr, out);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_sde_actor_set_batch_matrix(pgx_sde_actor_handle h, const float* in, void* stream) {
    const char* what = "pgx_sde_actor_set_batch_matrix";
    if (!h || !in) return fail(PGX_E_INVALID, what, "null handle or in pointer");
    hipLaunchKernelGGL(sde_batch_copy_kernel, dim3((h->a.H * h->a.ad + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->a,
                       h->bt, in, (float*)nullptr);
    return hipGetLastError() == hipSuccess ? PGX_OK : fail(PGX_E_HIP, what, "launch failed");
}

int pgx_sde_actor_batch_state(pgx_sde_actor_handle h, uint64_t* generation, void* stream) {
    if (!h || !generation)
        return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_batch_state: null handle or generation pointer");
    return read_word("pgx_sde_actor_batch_state", h->bt.gen, generation, stream);
}

int pgx_sde_actor_batch_set_state(pgx_sde_actor_handle h, uint64_t generation, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_batch_set_state: null handle");
    return write_word("pgx_sde_actor_batch_set_state", h->bt.gen, generation, stream);
}

int pgx_sde_actor_state(pgx_sde_actor_handle h, uint64_t* generation, void* stream) {
    if (!h || !generation) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_state: null handle or generation pointer");
    return read_word("pgx_sde_actor_state", h->a.gen, generation, stream);
}

int pgx_sde_actor_set_state(pgx_sde_actor_handle h, uint64_t generation, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_sde_actor_set_state: null handle");
    return write_word("pgx_sde_actor_set_state", h->a.gen, generation, stream);
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
                       h->a.std, out, n_std, (float*)nullptr, (float*)nullptr, h->a.ad);
    return hipGetLastError() == hipSuccess ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_sde_actor_get_std: launch failed");
}

}  // extern "C"
