/*
 * pgx_order_model.cpp -- host model of order_env (pgx_kernels.hip): the heavy-first env order a
 * wave of the per-pair manifold step kernels derives from the previous step's key bytes.
 *
 * 64-element arrays stand for the wave's lanes and every step is the device code's: the 16 key
 * bytes per lane in four words, the masked tail, the bisection for the first rank's bin, the byte
 * compares by carry, the DPP prefix sum (row_shr 1, 2, 4, 8, then row_bcast 15 and 31), the ballots
 * and the pick inside the lane by the 16 lanes of the env's row.  Built as libpgx_order_model.so
 * (Makefile) and checked on the CPU against numpy's stable argsort
 * (tests/test_env_order_model.py); no GPU, no HIP.
 */
#include <stdint.h>
#include <string.h>

namespace {
constexpr int WAVE = 64, GW = 16, EPW = WAVE / GW, KPL = 16;

int popc(uint32_t x) { return __builtin_popcount(x); }

/* x[l] += x[l - n] within the 16-lane row (DPP row_shr:n, 0 where the source is outside the row) */
void row_shr_add(int* x, int n) {
    int y[WAVE];
    for (int l = 0; l < WAVE; l++) y[l] = x[l] + ((l % 16) >= n ? x[l - n] : 0);
    memcpy(x, y, sizeof y);
}
/* x[l] += x[src row's last lane] for the rows of `rows` (DPP row_bcast:15 / row_bcast:31 with a row mask) */
void row_bcast_add(int* x, int which, unsigned rows) {
    int y[WAVE];
    for (int l = 0; l < WAVE; l++) {
        const int row = l / 16;
        const int src = which == 15 ? row * 16 - 1 : 31;
        y[l] = x[l] + (((rows >> row) & 1u) && src >= 0 ? x[src] : 0);
    }
    memcpy(x, y, sizeof y);
}
void wave_prefix_sum(int* x) {
    row_shr_add(x, 1);
    row_shr_add(x, 2);
    row_shr_add(x, 4);
    row_shr_add(x, 8);
    row_bcast_add(x, 15, 0xA);
    row_bcast_add(x, 31, 0xC);
}
uint64_t ballot(const bool* p) {
    uint64_t m = 0;
    for (int l = 0; l < WAVE; l++) m |= (uint64_t)p[l] << l;
    return m;
}
}  // namespace

/* the envs of block `block`'s EPW slots, out[t] for row t; keys: [N] bytes (read in 16-byte pieces:
 * padded to a multiple of 16); segs 1 or 8 (N a multiple of 8 x 256), as the launcher chooses */
/* top: the heaviest bin (the kernel's robot budget, order_env<TOP>) */
extern "C" void pgx_order_model(const uint8_t* keys, int N, int segs, int block, int top, int32_t* out) {
    const int S = segs == 1 ? N : N >> 3;
    const int base = segs == 1 ? 0 : (block & 7) * S;
    const int r0 = (segs == 1 ? block : block >> 3) * EPW;
    uint32_t kw[4][WAVE];
    for (int l = 0; l < WAVE; l++) {
        const int nv = S - KPL * l;
        for (int d = 0; d < 4; d++) kw[d][l] = 0u;
        if (nv > 0) {
            for (int d = 0; d < 4; d++) memcpy(&kw[d][l], keys + base + KPL * l + 4 * d, 4);
        }
        for (int d = 0; d < 4; d++) {
            const int nd = nv - 4 * d;
            kw[d][l] &= nd <= 0 ? 0u : 0x7f7f7f7fu >> (32 - 8 * (nd > 4 ? 4 : nd));
        }
    }
    int lo = 0, hi = top, B = 0;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const uint32_t up = 0x01010101u * (uint32_t)(0x80 - mid);
        int x[WAVE];
        for (int l = 0; l < WAVE; l++) {
            x[l] = 0;
            for (int d = 0; d < 4; d++) x[l] += popc((kw[d][l] + up) & 0x80808080u);
        }
        wave_prefix_sum(x);
        const int g = x[63];
        if (g > r0) {
            lo = mid;
        } else {
            hi = mid - 1;
            B = g;
        }
    }
    int lsel[WAVE], jsel[WAVE], ksel[WAVE];
    for (int l = 0; l < WAVE; l++) { lsel[l] = 0; jsel[l] = 0; ksel[l] = 0xff; }
    for (int k = lo; k >= 0; k--) {
        const uint32_t kk = 0x01010101u * (uint32_t)k;
        int c[WAVE], x[WAVE];
        for (int l = 0; l < WAVE; l++) {
            int nz = 0;
            for (int d = 0; d < 4; d++) nz += popc(((kw[d][l] ^ kk) + 0x7f7f7f7fu) & 0x80808080u);
            c[l] = KPL - nz;
            x[l] = c[l];
        }
        wave_prefix_sum(x);
        const int T = x[63];
        const int p0 = r0 - B;
        if (p0 < T && p0 + EPW > 0) {
            for (int t = 0; t < EPW; t++) {
                const int p = p0 + t;
                if (p >= 0 && p < T) {
                    bool in[WAVE];
                    for (int l = 0; l < WAVE; l++) in[l] = x[l] <= p;
                    int lt = __builtin_popcountll(ballot(in));
                    lt = lt > 63 ? 63 : lt;
                    const int j = p - (x[lt] - c[lt]);
                    for (int l = 0; l < WAVE; l++)
                        if (l / GW == t) { lsel[l] = lt; jsel[l] = j; ksel[l] = k; }
                }
            }
        }
        B += T;
        if (B >= r0 + EPW) break;
    }
    bool match[WAVE], hit[WAVE];
    for (int l = 0; l < WAVE; l++) {
        const int b = l & (KPL - 1);
        const uint32_t w = kw[b >> 2][lsel[l]];
        match[l] = (int)((w >> (8 * (b & 3))) & 0xffu) == ksel[l];
    }
    const uint64_t mm = ballot(match);
    for (int l = 0; l < WAVE; l++) {
        const int b = l & (KPL - 1), ln = l / GW;
        const uint32_t gm = (uint32_t)(mm >> (KPL * ln)) & 0xffffu;
        hit[l] = match[l] && popc(gm & ((1u << b) - 1u)) == jsel[l];
    }
    const uint64_t hm = ballot(hit);
    for (int t = 0; t < EPW; t++) {
        const int l = t * GW;
        const uint32_t gh = (uint32_t)(hm >> (KPL * t)) & 0xffffu;
        int i = base + KPL * lsel[l] + __builtin_ctz(gh | 0x10000u);
        i = i < base ? base : i;
        i = i > base + S - 1 ? base + S - 1 : i;
        out[t] = i;
    }
}
