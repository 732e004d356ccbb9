/*
 * pgx_monitor.hip -- device-resident VecMonitor (include/pgx.h, section "VecMonitor"):
 * stable-baselines3's VecMonitor over the step outputs of a batched env -- episode return, length
 * and outcome, a ring of the newest `window` finished episodes, running totals, and
 * evaluate_policy's per-env episode quota.
 *
 * Totals (and the ring head, which lives beside them) are kept twice, a ping-pong pair, with one
 * device word that says which half is current: pgx_norm.hip's idiom.  A step is two launches on
 * the caller's stream, nothing else (no allocation, no copy node, no hand-off between the
 * workgroups of one launch -- stream order alone carries slab counts to ring positions):
 *   accumulate_kernel  block s owns the fixed env slab s: per env ret += reward (one f32 add),
 *                      len += 1, speed += |EE velocity| (fp64); it writes the slab's number of
 *                      recorded episodes and its partial totals (fp64 sums in ascending env id)
 *                      into the handle's partial buffer.  Block 0 flips the current-half word,
 *                      which no block of this launch reads.
 *   record_kernel      block s prefix-sums the (<= 64) slab counts, ranks its finished envs (wave
 *                      ballot, an LDS scan across waves) and writes their records to
 *                      ring[(head + offset + rank) % window], head read from the previous half;
 *                      finished envs get ep_r / ep_l, ep_count + 1 and cleared accumulators.
 *                      Block 0 adds the slab partials in slab order to the previous half's totals
 *                      and stores them, head and step counter advanced, into the half that is now
 *                      current, which no block reads.
 * So a captured sequence of any length replays correctly: nothing the host passes depends on the
 * parity, the head or the step counter.
 *
 * Contraction is off for the unit (the speed's products are exact in fp64 either way).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/pgx.h"

#pragma clang fp contract(off)

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;
constexpr int WAVES = BLOCK / WAVE;
constexpr int MAX_SLABS = 64;
constexpr int MAX_WINDOW = 1 << 24;
constexpr int32_t NO_TARGET = INT32_MAX;

constexpr int W_CUR = 0;     /* control word: which half of the totals pair is current */

/* a slab's partial totals: integer counts, then the two fp64 sums */
enum { P_REC = 0, P_OUT0 = 1, P_LEN = 5, P_LEN_S = 6, P_OPEN = 7, P_INTS = 8 };
struct Partial {
    int64_t cnt[P_INTS];
    double ret_sum, speed_sum;
};

struct Half {
    pgx_monitor_totals t;
    int64_t head;            /* records ever appended: the next goes to ring[head % window] */
};

struct MonDev {
    int32_t N, od, window, speed_col;
    int32_t slab, n_slabs;   /* envs per slab (a multiple of BLOCK), slabs */
    double* speed;           /* [N] */
    double* ring_speed;      /* [window] */
    int64_t* ring_step;      /* [window] */
    Half* half;              /* [2] */
    Partial* partial;        /* [n_slabs] */
    float* ret;              /* [N] */
    int32_t* len;            /* [N] */
    int32_t* ep_count;       /* [N] */
    int32_t* target;         /* [N], NO_TARGET without a quota */
    float* ring_r;           /* [window] */
    int32_t* ring_l;
    int32_t* ring_env;
    int32_t* ring_outcome;
    uint32_t* ctrl;          /* [4] W_* */
};

__device__ __forceinline__ bool is_done(const pgx_monitor_io& io, int e) {
    return (io.terminated[e] | io.truncated[e]) != 0;
}

/* evaluate.py:250-267 behind the non-finite guard: the first match wins */
__device__ __forceinline__ int outcome_of(const pgx_monitor_io& io, int e, float ret) {
    if ((io.nonfinite && io.nonfinite[e] != 0) || !isfinite(ret)) return PGX_EP_NONFINITE;
    if (io.success[e] != 0) return PGX_EP_SUCCESS;
    if (io.task_truncated && io.task_truncated[e] != 0) return PGX_EP_COLLISION;
    return PGX_EP_TIMEOUT;
}

/* ---- launch 1: per-env accumulators, slab counts and partial totals, the parity flip ---- */
__global__ void __launch_bounds__(BLOCK) accumulate_kernel(MonDev d, pgx_monitor_io io) {
    __shared__ unsigned long long s_cnt[P_INTS];
    __shared__ unsigned long long s_mask[WAVES];
    __shared__ double s_ret[BLOCK];
    __shared__ double s_spd[BLOCK];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    if (s == 0 && tid == 0) d.ctrl[W_CUR] ^= 1u;   /* read by later launches only */
    if (tid < P_INTS) s_cnt[tid] = 0ull;
    const int row0 = s * d.slab;
    const int rows = min(d.slab, d.N - row0);
    double ret_sum = 0.0, speed_sum = 0.0;   /* thread 0: the slab's sums, ascending env */
    for (int c0 = 0; c0 < rows; c0 += BLOCK) {   /* block-uniform */
        __syncthreads();   /* s_cnt zeroed; the previous chunk's reads of s_ret / s_spd ended */
        const int r = c0 + tid;
        bool summed = false, open = false;
        if (r < rows) {
            const int e = row0 + r;
            const bool done = is_done(io, e);
            const float ret = d.ret[e] + io.reward[e];
            d.ret[e] = ret;
            const int len = d.len[e] + 1;
            d.len[e] = len;
            double speed = d.speed[e];
            if (d.speed_col >= 0) {
                const float* v = (done ? io.terminal_obs : io.obs) + (size_t)e * d.od + d.speed_col;
                const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
                speed = speed + sqrt(x * x + y * y + z * z);
                d.speed[e] = speed;
            }
            const int cnt = d.ep_count[e], tgt = d.target[e];
            const bool rec = done && cnt < tgt;
            open = cnt + (rec ? 1 : 0) < tgt;
            if (rec) {
                const int oc = outcome_of(io, e, ret);
                atomicAdd(&s_cnt[P_REC], 1ull);
                atomicAdd(&s_cnt[P_OUT0 + oc], 1ull);
                if (oc != PGX_EP_NONFINITE) {
                    atomicAdd(&s_cnt[P_LEN], (unsigned long long)len);
                    if (oc == PGX_EP_SUCCESS) atomicAdd(&s_cnt[P_LEN_S], (unsigned long long)len);
                    s_ret[tid] = (double)ret;
                    s_spd[tid] = oc == PGX_EP_SUCCESS ? speed : 0.0;
                    summed = true;
                }
            }
        }
        const unsigned long long m_sum = __ballot(summed), m_open = __ballot(open);
        if (lane == 0) {
            s_mask[wave] = m_sum;
            atomicAdd(&s_cnt[P_OPEN], (unsigned long long)__popcll(m_open));
        }
        __syncthreads();
        if (tid == 0)
            for (int w = 0; w < WAVES; w++)
                for (unsigned long long m = s_mask[w]; m; m &= m - 1) {
                    const int i = w * WAVE + (__ffsll((long long)m) - 1);
                    ret_sum += s_ret[i];
                    speed_sum += s_spd[i];
                }
    }
    __syncthreads();
    Partial& p = d.partial[s];
    if (tid < P_INTS) p.cnt[tid] = (int64_t)s_cnt[tid];
    if (tid == 0) {
        p.ret_sum = ret_sum;
        p.speed_sum = speed_sum;
    }
}

/* ---- launch 2: the records, ep_r / ep_l, cleared accumulators, the totals ---- */
__global__ void __launch_bounds__(BLOCK) record_kernel(MonDev d, pgx_monitor_io io) {
    __shared__ int s_wave[WAVES];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const uint32_t cur = d.ctrl[W_CUR] & 1u;
    const Half& prev = d.half[cur ^ 1u];
    int64_t before = 0, K = 0;   /* records of this step in the slabs before this one, in all */
    for (int i = 0; i < d.n_slabs; i++) {
        const int64_t c = d.partial[i].cnt[P_REC];
        before += i < s ? c : 0;
        K += c;
    }
    const int64_t head = prev.head, step = prev.t.steps + 1;
    const int64_t skip = K > d.window ? K - d.window : 0;   /* deque(maxlen): the last `window` survive */
    const int row0 = s * d.slab;
    const int rows = min(d.slab, d.N - row0);
    int64_t base = before;
    for (int c0 = 0; c0 < rows; c0 += BLOCK) {   /* block-uniform */
        const int r = c0 + tid, e = row0 + r;
        const bool in = r < rows;
        const bool done = in && is_done(io, e);
        const int cnt = in ? d.ep_count[e] : 0;
        const bool rec = done && cnt < d.target[e];
        const unsigned long long m = __ballot(rec);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int woff = 0, total = 0;
        for (int w = 0; w < WAVES; w++) {
            woff += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (done) {
            const float ret = d.ret[e];
            const int len = d.len[e];
            if (rec) {
                const int64_t j = base + woff + __popcll(m & ((1ull << lane) - 1ull));
                if (j >= skip) {
                    const int64_t pos = (head + j) % d.window;
                    d.ring_r[pos] = ret;
                    d.ring_l[pos] = len;
                    d.ring_env[pos] = e;
                    d.ring_outcome[pos] = outcome_of(io, e, ret);
                    d.ring_step[pos] = step;
                    d.ring_speed[pos] = d.speed[e];
                }
                d.ep_count[e] = cnt + 1;
            }
            if (io.ep_r) io.ep_r[e] = ret;
            if (io.ep_l) io.ep_l[e] = len;
            d.ret[e] = 0.0f;
            d.len[e] = 0;
            d.speed[e] = 0.0;
        }
        base += total;
        __syncthreads();   /* s_wave is rewritten by the next chunk */
    }
    if (s == 0 && tid == 0) {
        Half n = prev;
        int64_t open = 0;
        for (int i = 0; i < d.n_slabs; i++) {
            const Partial& p = d.partial[i];
            n.t.episodes += p.cnt[P_REC];
            for (int k = 0; k < 4; k++) n.t.outcomes[k] += p.cnt[P_OUT0 + k];
            n.t.length_sum += p.cnt[P_LEN];
            n.t.length_sum_success += p.cnt[P_LEN_S];
            open += p.cnt[P_OPEN];
            n.t.return_sum = n.t.return_sum + p.ret_sum;
            n.t.speed_sum_success = n.t.speed_sum_success + p.speed_sum;
        }
        n.t.envs_open = open;
        n.t.steps = step;
        n.head = head + K;
        d.half[cur] = n;   /* the half no block of this launch reads */
    }
}

/* ---- VecMonitor.reset: the masked envs' running episodes are abandoned ---- */
__global__ void __launch_bounds__(BLOCK) reset_kernel(MonDev d, const uint8_t* mask) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= d.N || (mask && mask[e] == 0)) return;
    d.ret[e] = 0.0f;
    d.len[e] = 0;
    d.speed[e] = 0.0;
}

__global__ void __launch_bounds__(BLOCK) clear_kernel(MonDev d) {
    const int n = max(d.N, d.window);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        if (i < d.N) {
            d.ret[i] = 0.0f;
            d.len[i] = 0;
            d.speed[i] = 0.0;
            d.ep_count[i] = 0;
        }
        if (i < d.window) {
            d.ring_r[i] = 0.0f;
            d.ring_l[i] = 0;
            d.ring_env[i] = 0;
            d.ring_outcome[i] = 0;
            d.ring_step[i] = 0;
            d.ring_speed[i] = 0.0;
        }
    }
}

/* one block, after a change of targets or a clear: envs_open into both halves (the next step
 * rewrites the one that is not current); clear: every other total and the head to zero first */
__global__ void __launch_bounds__(BLOCK) recount_kernel(MonDev d, int clear) {
    __shared__ unsigned long long s_open;
    const int tid = threadIdx.x;
    if (tid == 0) s_open = 0ull;
    __syncthreads();
    int open = 0;
    for (int e = tid; e < d.N; e += BLOCK) open += d.ep_count[e] < d.target[e] ? 1 : 0;
    atomicAdd(&s_open, (unsigned long long)open);
    __syncthreads();
    if (tid == 0)
        for (int h = 0; h < 2; h++) {
            if (clear) {
                Half z = {};
                d.half[h] = z;
            }
            d.half[h].t.envs_open = (int64_t)s_open;
        }
}

bool launched() { return hipGetLastError() == hipSuccess; }

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

struct pgx_monitor {
    MonDev d;
    void* blob;
    int device;
};

extern "C" {

int pgx_monitor_create(const pgx_monitor_config* cfg, int device, pgx_monitor_handle* out) {
    if (!cfg || !out) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_create: null config or handle pointer");
    if (cfg->n_envs <= 0) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_create: n_envs must be > 0");
    if (cfg->obs_dim <= 0) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_create: obs_dim must be > 0");
    if (cfg->window <= 0 || cfg->window > MAX_WINDOW)
        return pgx_set_error(PGX_E_INVALID, "pgx_monitor_create: window must be in [1, 2^24]");
    if (cfg->speed_col >= 0 && (int64_t)cfg->speed_col + 3 > cfg->obs_dim)
        return pgx_set_error(PGX_E_INVALID, "pgx_monitor_create: speed_col + 3 must be <= obs_dim");
    if (hipSetDevice(device) != hipSuccess) return pgx_set_error(PGX_E_HIP, "pgx_monitor_create: hipSetDevice");
    pgx_monitor* h = new pgx_monitor();
    MonDev& d = h->d;
    d.N = cfg->n_envs;
    d.od = cfg->obs_dim;
    d.window = cfg->window;
    d.speed_col = cfg->speed_col < 0 ? -1 : cfg->speed_col;
    const int per = (d.N + BLOCK * MAX_SLABS - 1) / (BLOCK * MAX_SLABS);
    d.slab = BLOCK * (per < 1 ? 1 : per);
    d.n_slabs = (d.N + d.slab - 1) / d.slab;
    const size_t N = (size_t)d.N, W = (size_t)d.window;
    /* one allocation: the 8-byte arrays first, then the 4-byte ones */
    size_t o = 0;
    const size_t o_speed = o;        o += N * sizeof(double);
    const size_t o_ring_speed = o;   o += W * sizeof(double);
    const size_t o_ring_step = o;    o += W * sizeof(int64_t);
    const size_t o_half = o;         o += 2 * sizeof(Half);
    const size_t o_partial = o;      o += (size_t)d.n_slabs * sizeof(Partial);
    const size_t o_ret = o;          o += N * 4;
    const size_t o_len = o;          o += N * 4;
    const size_t o_count = o;        o += N * 4;
    const size_t o_target = o;       o += N * 4;
    const size_t o_ring_r = o;       o += W * 4;
    const size_t o_ring_l = o;       o += W * 4;
    const size_t o_ring_env = o;     o += W * 4;
    const size_t o_ring_outcome = o; o += W * 4;
    const size_t o_ctrl = o;         o += 4 * sizeof(uint32_t);
    const size_t total = align8(o);
    h->device = device;
    if (hipMalloc(&h->blob, total) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_NOMEM, "pgx_monitor_create: hipMalloc failed");
    }
    char* b = (char*)h->blob;
    d.speed = (double*)(b + o_speed);
    d.ring_speed = (double*)(b + o_ring_speed);
    d.ring_step = (int64_t*)(b + o_ring_step);
    d.half = (Half*)(b + o_half);
    d.partial = (Partial*)(b + o_partial);
    d.ret = (float*)(b + o_ret);
    d.len = (int32_t*)(b + o_len);
    d.ep_count = (int32_t*)(b + o_count);
    d.target = (int32_t*)(b + o_target);
    d.ring_r = (float*)(b + o_ring_r);
    d.ring_l = (int32_t*)(b + o_ring_l);
    d.ring_env = (int32_t*)(b + o_ring_env);
    d.ring_outcome = (int32_t*)(b + o_ring_outcome);
    d.ctrl = (uint32_t*)(b + o_ctrl);
    /* everything zero; no targets, so every env is open */
    std::vector<char> init(total, 0);
    Half first = {};
    first.t.envs_open = d.N;
    memcpy(&init[o_half], &first, sizeof(Half));
    memcpy(&init[o_half + sizeof(Half)], &first, sizeof(Half));
    for (size_t e = 0; e < N; e++) memcpy(&init[o_target + 4 * e], &NO_TARGET, 4);
    if (hipMemcpy(h->blob, init.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(h->blob);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_monitor_create: hipMemcpy failed");
    }
    *out = h;
    return PGX_OK;
}

void pgx_monitor_destroy(pgx_monitor_handle h) {
    if (!h) return;
    (void)hipFree(h->blob);
    delete h;
}

int pgx_monitor_step(pgx_monitor_handle h, const pgx_monitor_io* io, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_step: null handle or io pointer");
    if (!io->reward || !io->success || !io->terminated || !io->truncated)
        return pgx_set_error(PGX_E_INVALID, "pgx_monitor_step: reward, success, terminated and truncated are required");
    const MonDev& d = h->d;
    if (d.speed_col >= 0 && (!io->obs || !io->terminal_obs))
        return pgx_set_error(PGX_E_INVALID, "pgx_monitor_step: obs and terminal_obs are required with speed_col >= 0");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(accumulate_kernel, dim3(d.n_slabs), dim3(BLOCK), 0, st, d, *io);
    hipLaunchKernelGGL(record_kernel, dim3(d.n_slabs), dim3(BLOCK), 0, st, d, *io);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_monitor_step: launch failed");
}

int pgx_monitor_reset(pgx_monitor_handle h, const uint8_t* mask, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_reset: null handle");
    hipLaunchKernelGGL(reset_kernel, dim3((h->d.N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, (hipStream_t)stream, h->d, mask);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_monitor_reset: launch failed");
}

int pgx_monitor_clear(pgx_monitor_handle h, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_clear: null handle");
    const MonDev& d = h->d;
    const int n = d.N > d.window ? d.N : d.window;
    int blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(clear_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, d);
    hipLaunchKernelGGL(recount_kernel, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, d, 1);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_monitor_clear: launch failed");
}

int pgx_monitor_set_targets(pgx_monitor_handle h, const int32_t* targets, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_set_targets: null handle");
    const MonDev& d = h->d;
    std::vector<int32_t> t(d.N, NO_TARGET);
    if (targets)
        for (int e = 0; e < d.N; e++) {
            if (targets[e] < 0) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_set_targets: targets must be >= 0");
            t[e] = targets[e];
        }
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_monitor_set_targets: hipStreamSynchronize");
    if (hipMemcpy(d.target, t.data(), (size_t)d.N * 4, hipMemcpyHostToDevice) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_monitor_set_targets: hipMemcpy");
    hipLaunchKernelGGL(recount_kernel, dim3(1), dim3(BLOCK), 0, (hipStream_t)stream, d, 0);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_monitor_set_targets: launch failed");
}

static int read_half(pgx_monitor_handle h, Half* out, void* stream, const char* what) {
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return pgx_set_error(PGX_E_HIP, what);
    uint32_t cur = 0;
    if (hipMemcpy(&cur, h->d.ctrl + W_CUR, sizeof(cur), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, what);
    if (hipMemcpy(out, h->d.half + (cur & 1u), sizeof(Half), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, what);
    return PGX_OK;
}

int pgx_monitor_get_totals(pgx_monitor_handle h, pgx_monitor_totals* out, void* stream) {
    if (!h || !out) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_get_totals: null handle or totals pointer");
    Half cur;
    const int rc = read_half(h, &cur, stream, "pgx_monitor_get_totals: device read failed");
    if (rc != PGX_OK) return rc;
    *out = cur.t;
    return PGX_OK;
}

int pgx_monitor_read(pgx_monitor_handle h, int32_t max, float* r, int32_t* l, int32_t* env, int32_t* outcome,
                     int64_t* step, double* speed_sum, int32_t* count, void* stream) {
    if (!h || !count) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_read: null handle or count pointer");
    if (max < 0) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_read: max < 0");
    const MonDev& d = h->d;
    const char* what = "pgx_monitor_read: device read failed";
    Half cur;
    const int rc = read_half(h, &cur, stream, what);
    if (rc != PGX_OK) return rc;
    const size_t W = (size_t)d.window;
    const int64_t retained = cur.head < d.window ? cur.head : d.window;
    const int64_t n = retained < max ? retained : max;
    *count = (int32_t)n;
    if (n == 0) return PGX_OK;
    std::vector<float> hr(W);
    std::vector<int32_t> hl(W), he(W), ho(W);
    std::vector<int64_t> hs(W);
    std::vector<double> hv(W);
    if ((r && hipMemcpy(hr.data(), d.ring_r, W * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (l && hipMemcpy(hl.data(), d.ring_l, W * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (env && hipMemcpy(he.data(), d.ring_env, W * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (outcome && hipMemcpy(ho.data(), d.ring_outcome, W * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (step && hipMemcpy(hs.data(), d.ring_step, W * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
        (speed_sum && hipMemcpy(hv.data(), d.ring_speed, W * 8, hipMemcpyDeviceToHost) != hipSuccess))
        return pgx_set_error(PGX_E_HIP, what);
    for (int64_t i = 0; i < n; i++) {
        const size_t pos = (size_t)((cur.head - n + i) % d.window);
        if (r) r[i] = hr[pos];
        if (l) l[i] = hl[pos];
        if (env) env[i] = he[pos];
        if (outcome) outcome[i] = ho[pos];
        if (step) step[i] = hs[pos];
        if (speed_sum) speed_sum[i] = hv[pos];
    }
    return PGX_OK;
}

int pgx_monitor_get_env_state(pgx_monitor_handle h, float* ret, int32_t* len, double* speed, int32_t* ep_count,
                              void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_monitor_get_env_state: null handle");
    const MonDev& d = h->d;
    const size_t N = (size_t)d.N;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_monitor_get_env_state: hipStreamSynchronize");
    if ((ret && hipMemcpy(ret, d.ret, N * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (len && hipMemcpy(len, d.len, N * 4, hipMemcpyDeviceToHost) != hipSuccess) ||
        (speed && hipMemcpy(speed, d.speed, N * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
        (ep_count && hipMemcpy(ep_count, d.ep_count, N * 4, hipMemcpyDeviceToHost) != hipSuccess))
        return pgx_set_error(PGX_E_HIP, "pgx_monitor_get_env_state: hipMemcpy");
    return PGX_OK;
}

}  // extern "C"
