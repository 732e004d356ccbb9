/*
 * pgx_policy.h -- the host side the policy units (pgx_actor.hip, pgx_actor_critic.hip, pgx_sde_actor.hip,
 * pgx_quantile_critic.hip) share: planning a stack of Linears, the tile choice (choose_tile for a launch, max_tile
 * for what fits at all, set_tile_lds for a batch kernel pair's dynamic LDS), the handle's one device allocation,
 * copy-and-pack of a Linear, the noise word's read and write, the launch of a kernel in its tile size.  The
 * device side: pgx_mlp.h.  Everything here has internal linkage: each unit compiles its own copy.
 */
#ifndef PGX_POLICY_H
#define PGX_POLICY_H

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "pgx_mlp.h"

int pgx_set_error(int code, const char* msg);  /* pgx_api.cpp: sets pgx_last_error() */

namespace {

/* What a forward workgroup may take of the CU's 160 KiB of LDS: 512 bytes stay for the kernels' static
 * words.  The Actor and the SdeActor, whose row stride is S = 16 j + 4, need mt (2048 j + 512) bytes, so
 * this bound and the whole 160 KiB admit the same widths: j <= 79 (mt = 1), j <= 39 (mt = 2). */
constexpr size_t LDS_LIMIT = 160 * 1024 - 512;

int fail(int code, const char* what, const char* text) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", what, text);
    return pgx_set_error(code, msg);
}

/* (out, in) of Linear l of the stack in_dim -> hidden[0 .. nl) -> head_out */
void linear_dims(int in_dim, const int32_t* hidden, int nl, int head_out, int l, int* out, int* in) {
    *in = l == 0 ? in_dim : hidden[l - 1];
    *out = l < nl ? hidden[l] : head_out;
}

/* Plans the stack's nl + 1 Linears: fills p, gives each its place in the packed parameters (*off,
 * floats, moved on) and in the plain copies (plain_w / plain_b [nl + 1], *n_plain, floats, moved on).
 * Returns the widest K16 of the Linears l >= first, 16 at the least. */
int plan_stack(MlpPlan* p, int in_dim, const int32_t* hidden, int nl, int head_out, int first, size_t* off,
               size_t* plain_w, size_t* plain_b, size_t* n_plain) {
    int widest = 16;
    p->n_linear = nl + 1;
    for (int l = 0; l <= nl; l++) {
        int o, in;
        linear_dims(in_dim, hidden, nl, head_out, l, &o, &in);
        p->nkb[l] = (in + 15) / 16;
        p->ntiles[l] = (o + 15) / 16;   /* the head: one tile up to 16 outputs, two for the quantile critics' 17..32 */
        p->woff[l] = (int32_t)*off;
        *off += (size_t)p->nkb[l] * p->ntiles[l] * 256;
        p->boff[l] = (int32_t)*off;
        *off += (size_t)p->ntiles[l] * 16;
        if (l >= first && p->nkb[l] * 16 > widest) widest = p->nkb[l] * 16;
        plain_w[l] = *n_plain;
        *n_plain += (size_t)o * in;
        plain_b[l] = *n_plain;
        *n_plain += (size_t)o;
    }
    return widest;
}

/* Env tiles of 16 per workgroup: 2 from two_from envs on (4096: each workgroup streams every weight once,
 * and at 4096 x [256, 256] the halved L2 traffic outweighs the halved workgroup count: DESIGN.md; the
 * quantile critics measured 2 ahead from 17 rows on) or as env_var (NULL: none) says, 16 or 32 envs; 1
 * where lds_bytes(2) does not fit; 0 where lds_bytes(1) does not */
template <class F>
int choose_tile(int n_envs, const char* env_var, F lds_bytes, int two_from = 4096) {
    int mt = n_envs >= two_from ? 2 : 1;
    if (env_var)
        if (const char* t = std::getenv(env_var)) mt = std::atoi(t) == 32 ? 2 : 1;
    if (lds_bytes(mt) > LDS_LIMIT) mt = 1;
    return lds_bytes(mt) > LDS_LIMIT ? 0 : mt;
}

/* the largest tile lds_bytes admits, whatever the batch and the environment say: 2, 1, or 0 for none */
template <class F>
int max_tile(F lds_bytes) {
    return choose_tile(17, nullptr, lds_bytes, 17);
}

/* The dynamic LDS of a batch launch's kernel pair, k1 (16 rows) and k2 (32), each for its own tile: 16 rows
 * where they fit, 32 where they do.  False: the runtime refused. */
template <class K, class F>
bool set_tile_lds(K k1, K k2, F lds_bytes) {
    const int mt_max = max_tile(lds_bytes);
    bool ok = true;
    for (int mt = 1; mt <= mt_max; mt++)
        ok = ok && hipFuncSetAttribute((const void*)(mt == 2 ? k2 : k1), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds_bytes(mt)) == hipSuccess;
    return ok;
}

/* The handle's one device allocation, zeroed: n regions of bytes[i], region i at the 256-aligned ptr[i]
 * (ptr[0] is what hipFree takes); and lds_bytes of dynamic LDS for every kernel of `kernels`.  On
 * failure nothing stays allocated and the error is set under `what`. */
int create_blob(const char* what, int device, const size_t* bytes, int n, void** ptr,
                std::initializer_list<const void*> kernels, size_t lds_bytes) {
    if (hipSetDevice(device) != hipSuccess) return fail(PGX_E_HIP, what, "hipSetDevice");
    size_t o[8], total = 0;
    for (int i = 0; i < n; i++) {
        o[i] = (total + 255) & ~(size_t)255;
        total = o[i] + bytes[i];
    }
    void* blob = nullptr;
    if (hipMalloc(&blob, total) != hipSuccess) return fail(PGX_E_NOMEM, what, "hipMalloc failed");
    bool ok = hipMemset(blob, 0, total) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    for (const void* k : kernels)
        ok = ok && hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
    if (!ok) {
        (void)hipFree(blob);
        return fail(PGX_E_HIP, what, "device setup failed");
    }
    for (int i = 0; i < n; i++) ptr[i] = (char*)blob + o[i];
    return PGX_OK;
}

/* One Linear's plain [out, in] weights and [out] bias into their packed place.  With staging (sw, sb:
 * the handle's plain copies; NULL: W and b are device memory, packed where they lie) they are copied
 * there first.  False: a copy failed. */
bool pack_linear(const float* W, const float* b, float* sw, float* sb, int out, int in, float* P, float* bp,
                 int ntiles, int row_off, hipStream_t st) {
    if (sw) {
        if (hipMemcpyAsync(sw, W, (size_t)out * in * 4, hipMemcpyDefault, st) != hipSuccess ||
            hipMemcpyAsync(sb, b, (size_t)out * 4, hipMemcpyDefault, st) != hipSuccess)
            return false;
        W = sw;
        b = sb;
    }
    const int n = out * in + out;
    hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, W, b, P, bp, out, in, ntiles, row_off);
    return true;
}

/* the noise word, behind everything enqueued on the stream */
int read_word(const char* what, const unsigned long long* word, uint64_t* out, void* stream) {
    unsigned long long v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(&v, word, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(PGX_E_HIP, what, "device read failed");
    *out = v;
    return PGX_OK;
}

int write_word(const char* what, unsigned long long* word, uint64_t value, void* stream) {
    const unsigned long long v = value;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
        hipMemcpy(word, &v, sizeof(v), hipMemcpyHostToDevice) != hipSuccess)
        return fail(PGX_E_HIP, what, "device write failed");
    return PGX_OK;
}

/* k1 (16 envs per workgroup) or k2 (32) over n envs */
template <class K, class... Args>
void launch_tiles(K k1, K k2, int mt, int n, size_t lds_bytes, void* stream, const Args&... args) {
    const int rows = mt * 16;
    hipLaunchKernelGGL(mt == 2 ? k2 : k1, dim3((n + rows - 1) / rows), dim3(THREADS), lds_bytes, (hipStream_t)stream,
                       args...);
}

}  // namespace

#endif /* PGX_POLICY_H */
