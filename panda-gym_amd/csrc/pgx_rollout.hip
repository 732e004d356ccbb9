/*
 * pgx_rollout.hip -- device-resident RolloutBuffer (include/pgx.h, section "RolloutBuffer"):
 * stable-baselines3's DictRolloutBuffer as OnPolicyAlgorithm.collect_rollouts fills it and
 * PPO.train reads it -- n_steps x n_envs transitions, the time-limit bootstrap, the GAE(lambda)
 * pass and get(batch_size)'s shuffled minibatches.
 *
 * Layout (HBM, one allocation): records [T][N][R], R = round_up(obs_dim + 6 + action_dim, 32)
 * floats -- observation | achieved_goal | desired_goal | action -- so a sampled transition's vector
 * fields are R * 4 contiguous bytes (pgx_her.hip's ring record); six dense f32 planes [T][N] for
 * reward, episode_start, value, log_prob, advantage and return, which the GAE pass walks one lane per
 * env (a wave reads 256 contiguous bytes per plane and step); the carry (SB3 _last_obs /
 * _last_episode_starts) as dense [N, .] arrays; the control words.
 *
 * Every entry point is one launch on the caller's stream, nothing else:
 *   add_kernel          16-lane groups, one per env: the carry and the action into the record at pos
 *                       with float4 stores, the scalars into the planes, the new carry.  pos is kept
 *                       once per workgroup of this kernel: each reads and advances its own copy, so
 *                       there is no hand-off between the workgroups of a launch (an agent-scope
 *                       fence writes a whole L2 back on this chip) and stream order alone carries pos
 *                       to the next launch; the copies are equal between launches and pos[0] is "pos".
 *   gae_kernel          one lane per env, sequential over t (a scan would re-associate); the loads
 *                       of a chunk of CH steps do not depend on the chain and are issued a chunk
 *                       ahead of it.
 *   permutation_kernel  one lane per output: the keyed Feistel walk of pgx.h.
 *   gather_kernel       16-lane groups, one per sample: float4 loads of the record, the four
 *                       scalars patched in behind it, float4 streaming stores of the row.
 *   reset_kernel / set_last_kernel
 *
 * Contraction is off for the unit: every f32 operation of the bootstrap and of GAE rounds on its own.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pgx.h"

#pragma clang fp contract(off)

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */

namespace {

constexpr int BLOCK = 256;
constexpr int GROUP = 16;                 /* lanes per record (one float4 each per pass) */
constexpr int PER_BLOCK = BLOCK / GROUP;  /* records per workgroup */
constexpr int GAE_BLOCK = 64;             /* one wave per workgroup: N / 64 workgroups over the CUs */
constexpr int CH = 8;                     /* GAE steps loaded ahead of the chain */

enum { W_ERRORS = 0, W_WORDS = 4 };
enum { P_REWARD = 0, P_START = 1, P_VALUE = 2, P_LOGP = 3, P_ADV = 4, P_RET = 5, P_PLANES = 6 };

struct RollDev {
    int32_t N, T, od, ad;
    int32_t V, R, S;         /* vector floats of a transition, record stride, batch row stride */
    float g, gl;             /* (float)gamma, (float)(gamma * gae_lambda) */
    float* rec;              /* [T][N][R] */
    float* plane;            /* [P_PLANES][T][N] */
    float *last_obs, *last_ag, *last_dg, *last_start;   /* the carry */
    int32_t* pos;            /* [n_pos]: one copy per add workgroup, all equal between launches */
    int32_t n_pos;
    uint32_t* ctrl;          /* [W_WORDS] */
};

struct PermKeys {
    uint32_t key[6];
    uint32_t k, mask, M;
};

__host__ __device__ inline uint32_t fmix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

PermKeys make_keys(uint64_t seed, uint64_t epoch, uint32_t M) {
    PermKeys p;
    uint32_t s = fmix((uint32_t)seed ^ 0x9E3779B9u);
    s = fmix(s ^ (uint32_t)(seed >> 32));
    s = fmix(s ^ (uint32_t)epoch);
    s = fmix(s ^ (uint32_t)(epoch >> 32));
    for (uint32_t r = 0; r < 6; r++) {
        s = fmix(s + 0x9E3779B9u * (r + 1));
        p.key[r] = s;
    }
    uint32_t top = M - 1 > 1 ? M - 1 : 1, bits = 0;
    while (top) {
        bits++;
        top >>= 1;
    }
    p.k = (bits + 1) / 2 > 1 ? (bits + 1) / 2 : 1;
    p.mask = (1u << p.k) - 1u;   /* k <= 16 for M < 2^31 */
    p.M = M;
    return p;
}

__device__ __forceinline__ float* plane(const RollDev& d, int which) {
    return d.plane + (size_t)which * d.T * d.N;
}

/* float f of env e's record: the carry's observation dict, then this step's action, zero padding */
__device__ __forceinline__ float record_value(const RollDev& d, const pgx_rollout_io& io, int e, int f) {
    if (f < d.od) return d.last_obs[(size_t)e * d.od + f];
    if (f < d.od + 3) return d.last_ag[(size_t)e * 3 + (f - d.od)];
    if (f < d.od + 6) return d.last_dg[(size_t)e * 3 + (f - d.od - 3)];
    if (f < d.V) return io.action[(size_t)e * d.ad + (f - d.od - 6)];
    return 0.0f;
}

/* ---------------------------------------------------------------- add */
__global__ void __launch_bounds__(BLOCK) add_kernel(RollDev d, pgx_rollout_io io) {
    const int tid = threadIdx.x, g = tid % GROUP;
    const int e = blockIdx.x * PER_BLOCK + tid / GROUP;
    const int32_t pos = d.pos[blockIdx.x];   /* this workgroup's copy: nobody else touches it */
    const bool room = pos < d.T;
    if (room && e < d.N) {
        const size_t se = (size_t)pos * d.N + e;
        float* rec = d.rec + se * d.R;
        /* a lane stores the new carry over the very floats it has just read: no other lane touches them */
        for (int c = g; 4 * c < d.R; c += GROUP) {
            float4 v;
            v.x = record_value(d, io, e, 4 * c + 0);
            v.y = record_value(d, io, e, 4 * c + 1);
            v.z = record_value(d, io, e, 4 * c + 2);
            v.w = record_value(d, io, e, 4 * c + 3);
            *reinterpret_cast<float4*>(rec + 4 * c) = v;
            if (io.obs)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int f = 4 * c + k;
                    if (f < d.od) d.last_obs[(size_t)e * d.od + f] = io.obs[(size_t)e * d.od + f];
                    else if (f < d.od + 3) d.last_ag[(size_t)e * 3 + (f - d.od)] = io.achieved_goal[(size_t)e * 3 + (f - d.od)];
                    else if (f < d.od + 6)
                        d.last_dg[(size_t)e * 3 + (f - d.od - 3)] = io.desired_goal[(size_t)e * 3 + (f - d.od - 3)];
                }
        }
        if (g == 0) {
            const bool te = io.terminated && io.terminated[e] != 0;
            const bool tr = io.truncated && io.truncated[e] != 0;
            float r = io.reward[e];
            if (io.terminal_value && tr && !te) {
                const float boot = d.g * io.terminal_value[e];
                r = r + boot;
            }
            plane(d, P_REWARD)[se] = r;
            plane(d, P_START)[se] = d.last_start[e];
            plane(d, P_VALUE)[se] = io.value[e];
            plane(d, P_LOGP)[se] = io.log_prob[e];
            if (io.obs) d.last_start[e] = (te || tr) ? 1.0f : 0.0f;
        }
    }
    __syncthreads();   /* every lane has read pos */
    if (tid == 0) {
        if (room) d.pos[blockIdx.x] = pos + 1;
        else atomicOr(&d.ctrl[W_ERRORS], (uint32_t)PGX_ROLLOUT_ERR_OVERFLOW);
    }
}

/* ---------------------------------------------------------------- GAE */
struct Chunk {
    float r[CH], v[CH], s[CH];   /* steps t0, t0 - 1, ..., t0 - CH + 1 (those >= 0) */
};

__device__ __forceinline__ void load_chunk(const RollDev& d, int e, int t0, Chunk& c) {
    const float* pr = plane(d, P_REWARD);
    const float* pv = plane(d, P_VALUE);
    const float* ps = plane(d, P_START);
#pragma unroll
    for (int i = 0; i < CH; i++) {
        const int t = t0 - i;
        const size_t at = (size_t)(t < 0 ? 0 : t) * d.N + e;   /* t < 0: loaded, never used */
        c.r[i] = pr[at];
        c.v[i] = pv[at];
        c.s[i] = ps[at];
    }
}

__global__ void __launch_bounds__(GAE_BLOCK) gae_kernel(RollDev d, const float* last_values, const float* dones) {
    const int e = blockIdx.x * GAE_BLOCK + threadIdx.x;
    if (d.pos[0] != d.T) {
        if (e == 0) atomicOr(&d.ctrl[W_ERRORS], (uint32_t)PGX_ROLLOUT_ERR_NOT_FULL);
        return;
    }
    if (e >= d.N) return;
    float* pa = plane(d, P_ADV);
    float* pt = plane(d, P_RET);
    float nv = last_values[e];
    float ns = dones ? dones[e] : d.last_start[e];
    float last = 0.0f;
    Chunk cur, nxt;
    load_chunk(d, e, d.T - 1, cur);
    for (int t0 = d.T - 1; t0 >= 0; t0 -= CH) {
        load_chunk(d, e, t0 - CH, nxt);   /* independent of the chain below: in flight during it */
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int t = t0 - i;
            if (t >= 0) {
                const float nnt = 1.0f - ns;
                const float gv = d.g * nv;
                const float delta = (cur.r[i] + gv * nnt) - cur.v[i];
                const float gn = d.gl * nnt;
                last = delta + gn * last;
                const size_t at = (size_t)t * d.N + e;
                pa[at] = last;
                pt[at] = last + cur.v[i];
                nv = cur.v[i];
                ns = cur.s[i];
            }
        }
        cur = nxt;
    }
}

/* ------------------------------------------------------- permutation */
__global__ void __launch_bounds__(BLOCK) permutation_kernel(PermKeys p, int32_t* out) {
    const uint32_t i = blockIdx.x * (uint32_t)BLOCK + threadIdx.x;
    if (i >= p.M) return;
    uint32_t x = i;
    do {
        uint32_t L = x >> p.k, R = x & p.mask;
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const uint32_t n = L ^ (fmix(R * 0x9E3779B1u + p.key[r]) & p.mask);
            L = R;
            R = n;
        }
        x = (L << p.k) | R;
    } while (x >= p.M);
    out[i] = (int32_t)x;
}

/* ------------------------------------------------------------ gather */
__global__ void __launch_bounds__(BLOCK) gather_kernel(RollDev d, const int32_t* indices, int64_t B, float* rows) {
    const int tid = threadIdx.x, g = tid % GROUP;
    const int64_t b = (int64_t)blockIdx.x * PER_BLOCK + tid / GROUP;
    if (b >= B) return;
    const int64_t p = indices[b];
    const bool ok = p >= 0 && p < (int64_t)d.T * d.N;
    if (!ok && g == 0) atomicOr(&d.ctrl[W_ERRORS], (uint32_t)PGX_ROLLOUT_ERR_INDEX);
    const int env = ok ? (int)(p / d.T) : 0, step = ok ? (int)(p % d.T) : 0;
    const size_t se = (size_t)step * d.N + env;
    const float* rec = d.rec + se * d.R;
    typedef float f4v __attribute__((ext_vector_type(4)));
    for (int c = g; 4 * c < d.S; c += GROUP) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok) {
            if (4 * c < d.V) v = *reinterpret_cast<const float4*>(rec + 4 * c);   /* 4 c + 3 < R: in the record */
            float* vv = reinterpret_cast<float*>(&v);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int f = 4 * c + k - d.V;   /* 0..3: old_value, old_log_prob, advantage, return */
                if (f >= 0) vv[k] = f < 4 ? plane(d, P_VALUE + f)[se] : 0.0f;
            }
        }
        /* streaming store: the batch is written once and read by the learner later */
        const f4v nv4 = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(nv4, reinterpret_cast<f4v*>(rows + b * d.S + 4 * c));
    }
}

/* ------------------------------------------------- reset / set_last */
__global__ void __launch_bounds__(BLOCK) reset_kernel(RollDev d) {
    for (int i = threadIdx.x; i < d.n_pos; i += BLOCK) d.pos[i] = 0;   /* one workgroup */
}

__global__ void __launch_bounds__(BLOCK) set_last_kernel(RollDev d, const float* obs, const float* ag, const float* dg,
                                                         const float* start) {
    const int W = d.od + 7;   /* floats of the carry per env */
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)d.N * W) return;
    const int e = (int)(i / W), f = (int)(i % W);
    if (f < d.od) d.last_obs[(size_t)e * d.od + f] = obs[(size_t)e * d.od + f];
    else if (f < d.od + 3) d.last_ag[(size_t)e * 3 + (f - d.od)] = ag[(size_t)e * 3 + (f - d.od)];
    else if (f < d.od + 6) d.last_dg[(size_t)e * 3 + (f - d.od - 3)] = dg[(size_t)e * 3 + (f - d.od - 3)];
    else d.last_start[e] = start ? start[e] : 1.0f;
}

/* create: everything zero, then the carry's episode_start at one */
__global__ void __launch_bounds__(BLOCK) init_kernel(size_t floats, float* blob) {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < floats; i += (size_t)gridDim.x * BLOCK) blob[i] = 0.0f;
}

__global__ void __launch_bounds__(BLOCK) ones_kernel(float* x, int n) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) x[i] = 1.0f;
}

bool launched() { return hipGetLastError() == hipSuccess; }

bool dims_ok(const pgx_rollout_config* c) {
    return c && c->n_envs > 0 && c->n_steps > 0 && c->obs_dim > 0 && c->action_dim > 0;
}

void make_dims(const pgx_rollout_config& c, RollDev& d) {
    d.N = c.n_envs;
    d.T = c.n_steps;
    d.od = c.obs_dim;
    d.ad = c.action_dim;
    d.V = d.od + 6 + d.ad;
    d.R = (d.V + 31) & ~31;
    d.S = (d.V + 4 + 3) & ~3;
    d.g = (float)c.gamma;
    d.gl = (float)(c.gamma * c.gae_lambda);
}

}  // namespace

struct pgx_rollout {
    RollDev d;
    pgx_rollout_config cfg;
    void* blob;
    int device;
};

extern "C" {

int pgx_rollout_row_dim(const pgx_rollout_config* cfg) {
    if (!dims_ok(cfg)) return PGX_E_INVALID;
    return cfg->obs_dim + 6 + cfg->action_dim + 4;
}

int pgx_rollout_row_stride(const pgx_rollout_config* cfg) {
    if (!dims_ok(cfg)) return PGX_E_INVALID;
    return (cfg->obs_dim + 6 + cfg->action_dim + 4 + 3) & ~3;
}

int pgx_rollout_create(const pgx_rollout_config* cfg, int device, pgx_rollout_handle* out) {
    if (!cfg || !out) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: null config or handle pointer");
    *out = nullptr;
    if (cfg->n_envs <= 0) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: n_envs must be > 0");
    if (cfg->n_steps <= 0) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: n_steps must be > 0");
    if (cfg->obs_dim <= 0 || cfg->obs_dim > (1 << 20))
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: obs_dim must be in [1, 2^20]");
    if (cfg->action_dim <= 0 || cfg->action_dim > (1 << 20))
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: action_dim must be in [1, 2^20]");
    if ((int64_t)cfg->n_steps * cfg->n_envs >= (1ll << 31))
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: n_steps * n_envs must be < 2^31");
    if (!(cfg->gamma >= 0.0 && cfg->gamma <= 1.0))
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: gamma must be in [0, 1]");
    if (!(cfg->gae_lambda >= 0.0 && cfg->gae_lambda <= 1.0))
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_create: gae_lambda must be in [0, 1]");
    if (hipSetDevice(device) != hipSuccess) return pgx_set_error(PGX_E_HIP, "pgx_rollout_create: hipSetDevice");
    pgx_rollout* h = new pgx_rollout();
    h->cfg = *cfg;
    h->device = device;
    RollDev& d = h->d;
    make_dims(*cfg, d);
    const size_t N = (size_t)d.N, M = N * (size_t)d.T;
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };   /* floats: 256-byte boundaries */
    d.n_pos = (d.N + PER_BLOCK - 1) / PER_BLOCK;
    const size_t sizes[] = {M * d.R, P_PLANES * M, N * d.od, N * 3, N * 3, N, (size_t)d.n_pos, (size_t)W_WORDS};
    size_t off[8], total = 0;
    for (int i = 0; i < 8; i++) {
        off[i] = total;
        total = al(total + sizes[i]);
    }
    if (hipMalloc(&h->blob, total * 4) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_NOMEM, "pgx_rollout_create: hipMalloc failed");
    }
    float* b = (float*)h->blob;
    d.rec = b + off[0];
    d.plane = b + off[1];
    d.last_obs = b + off[2];
    d.last_ag = b + off[3];
    d.last_dg = b + off[4];
    d.last_start = b + off[5];
    d.pos = (int32_t*)(b + off[6]);
    d.ctrl = (uint32_t*)(b + off[7]);
    /* zero everything (the records' padding stays zero for good), then episode_start = 1 */
    hipLaunchKernelGGL(init_kernel, dim3(1024), dim3(BLOCK), 0, 0, total, b);
    hipLaunchKernelGGL(ones_kernel, dim3((d.N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, d.last_start, d.N);
    if (!launched() || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(h->blob);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_rollout_create: initialisation failed");
    }
    *out = h;
    return PGX_OK;
}

void pgx_rollout_destroy(pgx_rollout_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipFree(h->blob);
    delete h;
}

int pgx_rollout_add(pgx_rollout_handle h, const pgx_rollout_io* io, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_add: null handle or io pointer");
    if (!io->action || !io->reward || !io->value || !io->log_prob)
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_add: action, reward, value and log_prob are required");
    if ((io->obs != nullptr) != (io->achieved_goal != nullptr) || (io->obs != nullptr) != (io->desired_goal != nullptr))
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_add: obs, achieved_goal and desired_goal go together");
    const RollDev& d = h->d;
    hipLaunchKernelGGL(add_kernel, dim3((d.N + PER_BLOCK - 1) / PER_BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, d, *io);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_rollout_add: launch failed");
}

int pgx_rollout_compute_returns_and_advantage(pgx_rollout_handle h, const float* last_values, const float* dones,
                                              void* stream) {
    if (!h || !last_values)
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_compute_returns_and_advantage: null handle or last_values");
    const RollDev& d = h->d;
    hipLaunchKernelGGL(gae_kernel, dim3((d.N + GAE_BLOCK - 1) / GAE_BLOCK), dim3(GAE_BLOCK), 0, (hipStream_t)stream, d,
                       last_values, dones);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_rollout_compute_returns_and_advantage: launch failed");
}

int pgx_rollout_permutation(pgx_rollout_handle h, uint64_t epoch, int32_t* out, void* stream) {
    if (!h || !out) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_permutation: null handle or output pointer");
    const uint32_t M = (uint32_t)((int64_t)h->d.N * h->d.T);
    const PermKeys p = make_keys(h->cfg.seed, epoch, M);
    hipLaunchKernelGGL(permutation_kernel, dim3((M + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, p, out);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_rollout_permutation: launch failed");
}

int pgx_rollout_gather(pgx_rollout_handle h, const int32_t* indices, int64_t batch, const pgx_rollout_batch* out,
                       void* stream) {
    if (!h || !indices || !out || !out->rows)
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_gather: null handle, indices or rows pointer");
    if (batch <= 0 || batch >= (1ll << 31)) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_gather: batch not in [1, 2^31)");
    if (((uintptr_t)out->rows & 15) != 0) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_gather: rows not 16 B aligned");
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((batch + PER_BLOCK - 1) / PER_BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)stream, h->d, indices, batch, out->rows);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_rollout_gather: launch failed");
}

int pgx_rollout_reset(pgx_rollout_handle h, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_reset: null handle");
    hipLaunchKernelGGL(reset_kernel, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, h->d);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_rollout_reset: launch failed");
}

int pgx_rollout_set_last(pgx_rollout_handle h, const float* obs, const float* achieved_goal, const float* desired_goal,
                         const float* episode_start, void* stream) {
    if (!h || !obs || !achieved_goal || !desired_goal)
        return pgx_set_error(PGX_E_INVALID, "pgx_rollout_set_last: null handle or observation pointer");
    const RollDev& d = h->d;
    const int64_t n = (int64_t)d.N * (d.od + 7);
    hipLaunchKernelGGL(set_last_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, d,
                       obs, achieved_goal, desired_goal, episode_start);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_rollout_set_last: launch failed");
}

int pgx_rollout_state(pgx_rollout_handle h, int32_t* pos, uint32_t* errors, int32_t clear, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_state: null handle");
    const char* what = "pgx_rollout_state: device read failed";
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return pgx_set_error(PGX_E_HIP, what);
    int32_t p = 0;
    uint32_t w[1] = {0u};
    if (hipMemcpy(&p, h->d.pos, sizeof(p), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(w, h->d.ctrl + W_ERRORS, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, what);
    if (pos) *pos = p;
    if (errors) *errors = w[0];
    if (clear && w[0] != 0u) {
        const uint32_t zero = 0u;
        if (hipMemcpy(h->d.ctrl + W_ERRORS, &zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess)
            return pgx_set_error(PGX_E_HIP, what);
    }
    return PGX_OK;
}

int pgx_rollout_arrays(pgx_rollout_handle h, pgx_rollout_views* out) {
    if (!h || !out) return pgx_set_error(PGX_E_INVALID, "pgx_rollout_arrays: null handle or views pointer");
    const RollDev& d = h->d;
    const size_t M = (size_t)d.N * d.T;
    out->records = d.rec;
    out->reward = d.plane + P_REWARD * M;
    out->episode_start = d.plane + P_START * M;
    out->value = d.plane + P_VALUE * M;
    out->log_prob = d.plane + P_LOGP * M;
    out->advantage = d.plane + P_ADV * M;
    out->returns = d.plane + P_RET * M;
    out->last_obs = d.last_obs;
    out->last_achieved_goal = d.last_ag;
    out->last_desired_goal = d.last_dg;
    out->last_episode_start = d.last_start;
    out->pos = d.pos;
    out->errors = d.ctrl + W_ERRORS;
    out->record_stride = d.R;
    out->pad0 = 0;
    return PGX_OK;
}

}  // extern "C"
