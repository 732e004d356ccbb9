/*
 * pgx_norm.hip -- device-resident VecNormalize (include/pgx.h, section "VecNormalize"):
 * stable-baselines3's VecNormalize / RunningMeanStd over the step outputs of a batched env.
 *
 * Statistics: per column fp64 mean / var / count, RunningMeanStd(epsilon = 1e-4).  A handle keeps
 * them twice (a ping-pong pair) and one device word that says which half is current.
 *
 * A step is two launches on the caller's stream, nothing else (no allocation, no copy node, no
 * hand-off between the workgroups of one launch -- stream order alone carries moments to
 * statistics to outputs):
 *   moments_kernel  grid (slabs, 4 keys): block (s, k) reduces key k's columns over the fixed env
 *                   slab s in fp64, two passes (mean, then squared deviations), and writes the
 *                   slab's (mean, M2) into the handle's partial buffer.  The returns key's blocks
 *                   run the returns recurrence first.  Block (0, 0) flips the current-half word,
 *                   which no block of this launch reads.
 *   apply_kernel    every block merges the partials in slab order with Chan's rule into the
 *                   previous half's statistics (each block the same operations, hence the same
 *                   bits), keeps the result in LDS and normalises its env rows; block 0 stores
 *                   the new statistics into the half that is now current, which no block reads.
 * So a captured sequence of any length replays correctly: nothing the host passes depends on the
 * parity, and whether statistics move at all (training) is a device word too.
 *
 * The whole unit is compiled with contraction off: given the statistics, every output is the
 * fp64 expression numpy evaluates, rounded once to f32 (fp64 / and sqrt are correctly rounded).
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
constexpr int MAX_OBS_DIM = BLOCK - 7;   /* obs_dim + 6 + 1 columns, one thread each in the merge */
constexpr int MAX_SLABS = 64;
constexpr int APPLY_ENVS = 64;           /* env rows per apply block */
constexpr int ROWS_PER_BLOCK = 64;       /* batch rows per pgx_norm_rows block */
constexpr int MAX_ROW_DIM = 2 * MAX_OBS_DIM + 14 + 64;

/* control words */
constexpr int W_CUR = 0;     /* which half of the statistics pair is current */
constexpr int W_TRAIN = 1;   /* statistics move (VecNormalize.training) */

struct NormDev {
    int32_t N, od, C;        /* C = od + 6 observation columns; column C = returns */
    int32_t slab, n_slabs;   /* envs per slab (a multiple of BLOCK), slabs */
    int32_t mask, norm_reward;
    int32_t reset;           /* this launch pair serves pgx_norm_reset */
    double clip_obs, clip_reward, gamma, epsilon;
    uint32_t* ctrl;          /* [2] W_* */
    double* stats;           /* [2][3][C + 1]: mean, var, count per half */
    double* partial;         /* [n_slabs][2][C + 1]: slab mean, slab M2 */
    double* returns;         /* [N] */
};

__device__ __forceinline__ int key_base(const NormDev& d, int key) {
    return key == 0 ? 0 : key == 1 ? d.od : key == 2 ? d.od + 3 : d.od + 6;
}
__device__ __forceinline__ int key_width(const NormDev& d, int key) { return key == 0 ? d.od : key == 3 ? 1 : 3; }
__device__ __forceinline__ int key_of_col(const NormDev& d, int c) {
    return c < d.od ? 0 : c < d.od + 3 ? 1 : c < d.od + 6 ? 2 : 3;
}

/* np.clip((x - mean) / np.sqrt(var + epsilon), -clip, clip).astype(np.float32), den = the sqrt */
__device__ __forceinline__ float norm_one(float x, double mean, double den, double clip) {
    double v = ((double)x - mean) / den;
    v = v < -clip ? -clip : v;
    v = v > clip ? clip : v;
    return (float)v;
}
/* np.clip(reward / np.sqrt(ret_var + epsilon), -clip, clip): no mean, so -0.0 stays -0.0 */
__device__ __forceinline__ float norm_reward_one(float x, double den, double clip) {
    double v = (double)x / den;
    v = v < -clip ? -clip : v;
    v = v > clip ? clip : v;
    return (float)v;
}
__device__ __forceinline__ float unnorm_one(float x, double mean, double den) { return (float)((double)x * den + mean); }
__device__ __forceinline__ float unnorm_reward_one(float x, double den) { return (float)((double)x * den); }

__device__ __forceinline__ const float* key_src(const pgx_norm_io& io, int key) {
    return key == 0 ? io.obs : key == 1 ? io.achieved_goal : io.desired_goal;
}

/* ---- launch 1: slab moments, the returns recurrence, the parity flip ---- */
__global__ void __launch_bounds__(BLOCK) moments_kernel(NormDev d, pgx_norm_io io) {
    __shared__ double red[BLOCK];
    __shared__ double col_mean[BLOCK];
    const int key = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
    const bool training = d.ctrl[W_TRAIN] != 0;
    if (s == 0 && key == 0 && tid == 0 && training) d.ctrl[W_CUR] ^= 1u;   /* read by later launches only */
    const int row0 = s * d.slab;
    const int rows = min(d.slab, d.N - row0);
    const int w = key_width(d, key);
    const int R = BLOCK / w;             /* row groups: thread (g, c) = (tid / w, tid % w) sums rows g, g + R, ... */
    const int g = tid / w, c = tid - g * w;
    const bool active = g < R;
    if (key == 3) {
        /* returns = returns * gamma + reward (reset: 0).  w = 1: thread tid owns rows tid, tid + BLOCK, ...
         * in this pass and in the two below, so it reads back what it stored itself.  A finished
         * env's returns are zeroed by the apply launch, after they have entered the moments. */
        for (int r = tid; r < rows; r += BLOCK) {
            const int e = row0 + r;
            d.returns[e] = d.reset ? 0.0 : d.returns[e] * d.gamma + (double)io.reward[e];
        }
    }
    const bool update = training && (key == 3 ? !d.reset : ((d.mask >> key) & 1) != 0);
    if (!update) return;   /* block-uniform */
    const float* src = key == 3 ? nullptr : key_src(io, key) + (size_t)row0 * w;
    const double* rsrc = d.returns + row0;
    double sum = 0.0;
    if (active)
        for (int r = g; r < rows; r += R) sum += key == 3 ? rsrc[r] : (double)src[(size_t)r * w + c];
    red[tid] = sum;
    __syncthreads();
    double mean = 0.0;
    if (tid < w) {
        double t = 0.0;
        for (int i = 0; i < R; i++) t += red[i * w + tid];
        mean = t / (double)rows;
        col_mean[tid] = mean;
    }
    __syncthreads();
    double q = 0.0;
    if (active) {
        const double m = col_mean[c];
        for (int r = g; r < rows; r += R) {
            const double x = key == 3 ? rsrc[r] : (double)src[(size_t)r * w + c];
            q += (x - m) * (x - m);
        }
    }
    red[tid] = q;   /* (pass 1's reads of red ended before the barrier above) */
    __syncthreads();
    if (tid < w) {
        double t = 0.0;
        for (int i = 0; i < R; i++) t += red[i * w + tid];
        const int col = key_base(d, key) + tid;
        d.partial[((size_t)s * 2 + 0) * (d.C + 1) + col] = mean;
        d.partial[((size_t)s * 2 + 1) * (d.C + 1) + col] = t;
    }
}

/* Column c's statistics after this step's update (every block the same bits): Chan's merge of the
 * slab partials in slab order, then RunningMeanStd.update_from_moments. */
__device__ __forceinline__ void merged_stats(const NormDev& d, int c, bool training, uint32_t cur, double& mean,
                                             double& var, double& count) {
    const int S = d.C + 1;
    const double* old = d.stats + (size_t)(training ? cur ^ 1u : cur) * 3 * S;
    mean = old[c];
    var = old[S + c];
    count = old[2 * S + c];
    const int key = key_of_col(d, c);
    const bool update = training && (key == 3 ? !d.reset : ((d.mask >> key) & 1) != 0);
    if (!update) return;
    double bn = 0.0, bmean = 0.0, bM2 = 0.0;
    for (int s = 0; s < d.n_slabs; s++) {
        const double n = (double)min(d.slab, d.N - s * d.slab);
        const double pm = d.partial[((size_t)s * 2 + 0) * S + c], pM2 = d.partial[((size_t)s * 2 + 1) * S + c];
        const double delta = pm - bmean, tot = bn + n;
        bmean = bmean + delta * n / tot;
        bM2 = bM2 + pM2 + delta * delta * bn * n / tot;
        bn = tot;
    }
    const double bvar = bM2 / bn;
    const double delta = bmean - mean, tot = count + bn;
    const double new_mean = mean + delta * bn / tot;
    const double M2 = var * count + bvar * bn + delta * delta * count * bn / tot;
    mean = new_mean;
    var = M2 / tot;
    count = tot;
}

/* ---- launch 2: statistics, normalised outputs ---- */
__global__ void __launch_bounds__(BLOCK) apply_kernel(NormDev d, pgx_norm_io io) {
    __shared__ double s_mean[BLOCK];
    __shared__ double s_den[BLOCK];
    const int tid = threadIdx.x;
    const bool training = d.ctrl[W_TRAIN] != 0;
    const uint32_t cur = d.ctrl[W_CUR] & 1u;
    const int S = d.C + 1;
    if (tid < S) {
        double mean, var, count;
        merged_stats(d, tid, training, cur, mean, var, count);
        s_mean[tid] = mean;
        s_den[tid] = sqrt(var + d.epsilon);
        if (blockIdx.x == 0 && training) {   /* the half no block of this launch reads */
            double* cs = d.stats + (size_t)cur * 3 * S;
            cs[tid] = mean;
            cs[S + tid] = var;
            cs[2 * S + tid] = count;
        }
    }
    __syncthreads();
    const int row0 = blockIdx.x * APPLY_ENVS;
    const int nr = min(APPLY_ENVS, d.N - row0);
    const uint8_t* term = io.terminated;
    const uint8_t* trunc = io.truncated;
#pragma unroll
    for (int key = 0; key < 3; key++) {
        const int w = key_width(d, key), base = key_base(d, key);
        const bool on = ((d.mask >> key) & 1) != 0;
        const float* src = key_src(io, key);
        float* dst = key == 0 ? io.out_obs : key == 1 ? io.out_achieved_goal : io.out_desired_goal;
        const float* tsrc = key == 0 ? io.terminal_obs : key == 1 ? io.terminal_achieved_goal : io.terminal_desired_goal;
        float* tdst = key == 0 ? io.out_terminal_obs : key == 1 ? io.out_terminal_achieved_goal
                                                                : io.out_terminal_desired_goal;
        const bool terminal = !d.reset && tsrc && tdst;
        for (int e = tid; e < nr * w; e += BLOCK) {
            const int r = e / w, c = e - r * w;
            const size_t idx = (size_t)row0 * w + e;
            const double m = s_mean[base + c], den = s_den[base + c];
            if (dst) {
                const float x = src[idx];
                dst[idx] = on ? norm_one(x, m, den, d.clip_obs) : x;
            }
            if (terminal && ((term[row0 + r] | trunc[row0 + r]) != 0)) {
                const float x = tsrc[idx];
                tdst[idx] = on ? norm_one(x, m, den, d.clip_obs) : x;
            }
        }
    }
    if (!d.reset && tid < nr) {
        const int e = row0 + tid;
        if (io.out_reward) {
            const float x = io.reward[e];
            io.out_reward[e] = d.norm_reward ? norm_reward_one(x, s_den[d.C], d.clip_reward) : x;
        }
        if ((term[e] | trunc[e]) != 0) d.returns[e] = 0.0;   /* VecNormalize.step_wait: returns[dones] = 0 */
    }
    if (io.flags && io.out_flags)   /* [flag_rows][N] u8, carried along so one copy brings a step to the host */
        for (int i = tid; i < io.flag_rows * nr; i += BLOCK) {
            const int f = i / nr, r = i - f * nr;
            io.out_flags[(size_t)f * d.N + row0 + r] = io.flags[(size_t)f * d.N + row0 + r];
        }
}

/* ---- a HER batch in place, current statistics, no update ---- */
__global__ void __launch_bounds__(BLOCK) rows_kernel(NormDev d, float* rows, int64_t batch, int32_t ad,
                                                     int32_t row_dim, int32_t row_stride) {
    __shared__ double t_mean[MAX_ROW_DIM];
    __shared__ double t_den[MAX_ROW_DIM];
    __shared__ uint8_t t_kind[MAX_ROW_DIM];   /* 0 untouched, 1 observation column, 2 reward */
    const int tid = threadIdx.x, S = d.C + 1, od = d.od;
    const double* cs = d.stats + (size_t)(d.ctrl[W_CUR] & 1u) * 3 * S;
    /* obs[od] | ag[3] | dg[3] | action[ad] | reward | next_obs[od] | next_ag[3] | next_dg[3] | done */
    for (int j = tid; j < row_dim; j += BLOCK) {
        int col = -1, kind = 0;
        if (j < od + 6) col = j;
        else if (j == od + 6 + ad) col = d.C;
        else if (j > od + 6 + ad && j < row_dim - 1) col = j - (od + 6 + ad + 1);
        if (col == d.C) kind = d.norm_reward ? 2 : 0;
        else if (col >= 0) kind = ((d.mask >> key_of_col(d, col)) & 1) ? 1 : 0;
        t_kind[j] = (uint8_t)kind;
        t_mean[j] = kind ? cs[col] : 0.0;
        t_den[j] = kind ? sqrt(cs[S + col] + d.epsilon) : 1.0;
    }
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK;
    const int nr = (int)min((int64_t)ROWS_PER_BLOCK, batch - r0);
    float* p = rows + r0 * row_stride;
    for (int e = tid; e < nr * row_stride; e += BLOCK) {
        const int j = e % row_stride;
        if (j >= row_dim) continue;
        const int kind = t_kind[j];
        if (kind == 1) p[e] = norm_one(p[e], t_mean[j], t_den[j], d.clip_obs);
        else if (kind == 2) p[e] = norm_reward_one(p[e], t_den[j], d.clip_reward);
    }
}

/* ---- stateless apply / inverse over [m, width] of one key (3: rewards, width 1) ---- */
__global__ void __launch_bounds__(BLOCK) apply_rows_kernel(NormDev d, int32_t key, int32_t inverse, const float* in,
                                                           float* out, int64_t total) {
    __shared__ double s_mean[BLOCK];
    __shared__ double s_den[BLOCK];
    const int tid = threadIdx.x, S = d.C + 1;
    const int w = key_width(d, key), base = key_base(d, key);
    const double* cs = d.stats + (size_t)(d.ctrl[W_CUR] & 1u) * 3 * S;
    if (tid < w) {
        s_mean[tid] = cs[base + tid];
        s_den[tid] = sqrt(cs[S + base + tid] + d.epsilon);
    }
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * BLOCK + tid; e < total; e += (int64_t)gridDim.x * BLOCK) {
        const int c = (int)(e % w);
        const float x = in[e];
        float y;
        if (key == 3) y = inverse ? unnorm_reward_one(x, s_den[0]) : norm_reward_one(x, s_den[0], d.clip_reward);
        else y = inverse ? unnorm_one(x, s_mean[c], s_den[c]) : norm_one(x, s_mean[c], s_den[c], d.clip_obs);
        out[e] = y;
    }
}

__global__ void set_word_kernel(uint32_t* ctrl, int word, uint32_t value) { ctrl[word] = value; }

bool launched() { return hipGetLastError() == hipSuccess; }

}  // namespace

struct pgx_norm {
    NormDev d;
    void* blob;
    int device;
};

extern "C" {

int pgx_norm_create(const pgx_norm_config* cfg, int device, pgx_norm_handle* out) {
    if (!cfg || !out) return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: null config or handle pointer");
    if (cfg->n_envs <= 0) return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: n_envs must be > 0");
    if (cfg->obs_dim <= 0 || cfg->obs_dim > MAX_OBS_DIM)
        return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: obs_dim must be in [1, 249]");
    if (!(cfg->epsilon >= 0.0)) return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: epsilon must be >= 0");
    if (cfg->key_mask < 0 || cfg->key_mask > PGX_NORM_KEY_ALL)
        return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: key_mask has unknown bits");
    if (!(cfg->clip_obs > 0.0) || !(cfg->clip_reward > 0.0))
        return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: clip_obs and clip_reward must be > 0");
    if (!(cfg->gamma >= 0.0)) return pgx_set_error(PGX_E_INVALID, "pgx_norm_create: gamma must be >= 0");
    if (hipSetDevice(device) != hipSuccess) return pgx_set_error(PGX_E_HIP, "pgx_norm_create: hipSetDevice");
    pgx_norm* h = new pgx_norm();
    NormDev& d = h->d;
    d.N = cfg->n_envs;
    d.od = cfg->obs_dim;
    d.C = cfg->obs_dim + 6;
    const int per = (d.N + BLOCK * MAX_SLABS - 1) / (BLOCK * MAX_SLABS);
    d.slab = BLOCK * (per < 1 ? 1 : per);
    d.n_slabs = (d.N + d.slab - 1) / d.slab;
    d.mask = cfg->key_mask;
    d.norm_reward = cfg->norm_reward != 0;
    d.reset = 0;
    d.clip_obs = cfg->clip_obs;
    d.clip_reward = cfg->clip_reward;
    d.gamma = cfg->gamma;
    d.epsilon = cfg->epsilon;
    const size_t S = (size_t)d.C + 1;
    const size_t n_stats = 2 * 3 * S, n_partial = (size_t)d.n_slabs * 2 * S;
    const size_t n_doubles = n_stats + n_partial + (size_t)d.N;
    const size_t total = n_doubles * sizeof(double) + 16;
    h->device = device;
    if (hipMalloc(&h->blob, total) != hipSuccess) {
        delete h;
        return pgx_set_error(PGX_E_NOMEM, "pgx_norm_create: hipMalloc failed");
    }
    d.stats = (double*)h->blob;
    d.partial = d.stats + n_stats;
    d.returns = d.partial + n_partial;
    d.ctrl = (uint32_t*)(d.returns + d.N);
    /* RunningMeanStd(epsilon=1e-4): mean 0, var 1, count 1e-4, in both halves; returns 0; training on */
    std::vector<double> init(n_doubles + 2, 0.0);
    for (int half = 0; half < 2; half++)
        for (size_t c = 0; c < S; c++) {
            init[(half * 3 + 1) * S + c] = 1.0;
            init[(half * 3 + 2) * S + c] = 1e-4;
        }
    uint32_t ctrl[4] = {0u, 1u, 0u, 0u};
    memcpy(&init[n_doubles], ctrl, sizeof(ctrl));
    if (hipMemcpy(h->blob, init.data(), total, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(h->blob);
        delete h;
        return pgx_set_error(PGX_E_HIP, "pgx_norm_create: hipMemcpy failed");
    }
    *out = h;
    return PGX_OK;
}

void pgx_norm_destroy(pgx_norm_handle h) {
    if (!h) return;
    (void)hipFree(h->blob);
    delete h;
}

static int norm_launch(pgx_norm_handle h, const pgx_norm_io* io, int reset, void* stream, const char* what) {
    NormDev d = h->d;
    d.reset = reset;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(moments_kernel, dim3(d.n_slabs, 4), dim3(BLOCK), 0, st, d, *io);
    hipLaunchKernelGGL(apply_kernel, dim3((d.N + APPLY_ENVS - 1) / APPLY_ENVS), dim3(BLOCK), 0, st, d, *io);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, what);
}

int pgx_norm_step(pgx_norm_handle h, const pgx_norm_io* io, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_norm_step: null handle or io pointer");
    if (!io->obs || !io->achieved_goal || !io->desired_goal || !io->reward || !io->terminated || !io->truncated)
        return pgx_set_error(PGX_E_INVALID, "pgx_norm_step: obs, goals, reward, terminated and truncated are required");
    if (io->flag_rows < 0) return pgx_set_error(PGX_E_INVALID, "pgx_norm_step: flag_rows < 0");
    return norm_launch(h, io, 0, stream, "pgx_norm_step: launch failed");
}

int pgx_norm_reset(pgx_norm_handle h, const pgx_norm_io* io, void* stream) {
    if (!h || !io) return pgx_set_error(PGX_E_INVALID, "pgx_norm_reset: null handle or io pointer");
    if (!io->obs || !io->achieved_goal || !io->desired_goal)
        return pgx_set_error(PGX_E_INVALID, "pgx_norm_reset: obs and goals are required");
    pgx_norm_io r = *io;
    r.flags = nullptr;
    r.out_flags = nullptr;
    r.flag_rows = 0;
    return norm_launch(h, &r, 1, stream, "pgx_norm_reset: launch failed");
}

int pgx_norm_rows(pgx_norm_handle h, float* rows, int64_t batch, int32_t action_dim, int32_t row_stride, void* stream) {
    if (!h || !rows) return pgx_set_error(PGX_E_INVALID, "pgx_norm_rows: null handle or rows pointer");
    const int64_t row_dim = 2 * (int64_t)h->d.od + action_dim + 14;
    if (batch < 1 || batch > ((int64_t)1 << 26) || action_dim < 1 || row_dim > MAX_ROW_DIM || row_stride < row_dim)
        return pgx_set_error(PGX_E_INVALID,
                             "pgx_norm_rows: batch not in [1, 2^26], or action_dim / row_stride do not fit the row layout");
    hipLaunchKernelGGL(rows_kernel, dim3((unsigned)((batch + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)stream, h->d, rows, batch, action_dim, (int32_t)row_dim, row_stride);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_norm_rows: launch failed");
}

int pgx_norm_apply(pgx_norm_handle h, int32_t key, int32_t inverse, const float* in, float* out, int64_t m, void* stream) {
    if (!h || !in || !out) return pgx_set_error(PGX_E_INVALID, "pgx_norm_apply: null handle or array pointer");
    if (key < 0 || key > PGX_NORM_REWARD) return pgx_set_error(PGX_E_INVALID, "pgx_norm_apply: unknown key");
    if (m < 0 || m > ((int64_t)1 << 40)) return pgx_set_error(PGX_E_INVALID, "pgx_norm_apply: bad row count");
    if (m == 0) return PGX_OK;
    const int w = key == 0 ? h->d.od : key == PGX_NORM_REWARD ? 1 : 3;
    const int64_t total = m * w;
    int64_t blocks = (total + BLOCK - 1) / BLOCK;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(apply_rows_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, h->d, key,
                       inverse != 0, in, out, total);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_norm_apply: launch failed");
}

int pgx_norm_set_training(pgx_norm_handle h, int32_t training, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_norm_set_training: null handle");
    hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, h->d.ctrl, W_TRAIN,
                       training ? 1u : 0u);
    return launched() ? PGX_OK : pgx_set_error(PGX_E_HIP, "pgx_norm_set_training: launch failed");
}

int pgx_norm_set_keys(pgx_norm_handle h, int32_t key_mask, int32_t norm_reward) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_norm_set_keys: null handle");
    if (key_mask < 0 || key_mask > PGX_NORM_KEY_ALL)
        return pgx_set_error(PGX_E_INVALID, "pgx_norm_set_keys: key_mask has unknown bits");
    h->d.mask = key_mask;
    h->d.norm_reward = norm_reward != 0;
    return PGX_OK;
}

int pgx_norm_get_stats(pgx_norm_handle h, double* mean, double* var, double* count, double* returns, void* stream) {
    if (!h) return pgx_set_error(PGX_E_INVALID, "pgx_norm_get_stats: null handle");
    const NormDev& d = h->d;
    const size_t S = (size_t)d.C + 1;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_get_stats: hipStreamSynchronize");
    uint32_t ctrl[2];
    if (hipMemcpy(ctrl, d.ctrl, sizeof(ctrl), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_get_stats: hipMemcpy");
    std::vector<double> half(3 * S);
    if (hipMemcpy(half.data(), d.stats + (size_t)(ctrl[W_CUR] & 1u) * 3 * S, 3 * S * sizeof(double),
                  hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_get_stats: hipMemcpy");
    if (mean) memcpy(mean, half.data(), S * sizeof(double));
    if (var) memcpy(var, half.data() + S, S * sizeof(double));
    if (count) memcpy(count, half.data() + 2 * S, S * sizeof(double));
    if (returns && hipMemcpy(returns, d.returns, (size_t)d.N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_get_stats: hipMemcpy");
    return PGX_OK;
}

int pgx_norm_set_stats(pgx_norm_handle h, const double* mean, const double* var, const double* count,
                       const double* returns, void* stream) {
    if (!h || !mean || !var || !count) return pgx_set_error(PGX_E_INVALID, "pgx_norm_set_stats: null handle or array");
    const NormDev& d = h->d;
    const size_t S = (size_t)d.C + 1;
    for (size_t c = 0; c < S; c++)
        if (!(var[c] >= 0.0) || !(count[c] > 0.0))
            return pgx_set_error(PGX_E_INVALID, "pgx_norm_set_stats: var must be >= 0 and count > 0");
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_set_stats: hipStreamSynchronize");
    std::vector<double> both(2 * 3 * S);
    for (int half = 0; half < 2; half++) {
        memcpy(&both[(half * 3 + 0) * S], mean, S * sizeof(double));
        memcpy(&both[(half * 3 + 1) * S], var, S * sizeof(double));
        memcpy(&both[(half * 3 + 2) * S], count, S * sizeof(double));
    }
    if (hipMemcpy(d.stats, both.data(), both.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_set_stats: hipMemcpy");
    if (returns && hipMemcpy(d.returns, returns, (size_t)d.N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return pgx_set_error(PGX_E_HIP, "pgx_norm_set_stats: hipMemcpy");
    return PGX_OK;
}

}  // extern "C"
