// Host checks of what the DAPOL_PREP=v2 digit producers rest on (dapol_amd/csrc/sc.h compiled for the CPU; stand-alone, built with
// -fsanitize=address,undefined by tests/test_prep_scalars_cpu.py):
//   1. sc_recode_fixed<17, 15> / <16, 16> (and two more geometries) give sc_recode_w's digits for random canonical scalars and for
//      scalars on every edge of the recoding: 0, 1, l - 1, 2^(W i) - 1 / + 0 / + 1 for every window boundary, and a carry running
//      through all windows with the boundary window pushed either way;
//   2. the shared fold scalars: for N = 32, random y and u_0..u_4 and every number of rounds r = 1..4 before a tail of length
//      T = N / 2^r, c_k * y^-i with c_k = y^-kT TH_r[k] equals the plain coefficient y^-j TH_r[j >> (lgN - r)] of generator
//      j = i + k T, for every j -- what k_rp_mat_prep_gs_shared writes times what the tail's s2 holds, against coeff_plain.
// Prints "ok <checks>" and exits 0, or says what differs and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sc.h"

using namespace dapol;

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd64() {
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static void rnd_sc(sc& r) {                       // a random scalar, Montgomery form
    uint32_t w[16];
    for (int i = 0; i < 16; i += 2) { const uint64_t x = rnd64(); w[i] = (uint32_t)x; w[i + 1] = (uint32_t)(x >> 32); }
    sc_from_wide(r, w);
}

struct U256 { uint32_t v[8]; };
static U256 u_zero() { U256 r; memset(r.v, 0, sizeof r.v); return r; }
static U256 u_pow2(int bit) { U256 r = u_zero(); r.v[bit >> 5] = 1u << (bit & 31); return r; }
static U256 u_add(const U256& a, const U256& b) {
    U256 r; uint64_t c = 0;
    for (int i = 0; i < 8; i++) { c += (uint64_t)a.v[i] + b.v[i]; r.v[i] = (uint32_t)c; c >>= 32; }
    return r;
}
static U256 u_sub(const U256& a, const U256& b) {
    U256 r; int64_t c = 0;
    for (int i = 0; i < 8; i++) { c += (int64_t)a.v[i] - (int64_t)b.v[i]; r.v[i] = (uint32_t)c; c >>= 32; }
    return r;
}
static bool u_below_l(const U256& a) {
    for (int i = 7; i >= 0; i--) if (a.v[i] != SC_L[i]) return a.v[i] < SC_L[i];
    return false;
}

static long g_checks = 0;

template <int W, int NW>
static bool recode_same(const U256& x, const char* what) {
    int a[NW], b[NW];
    sc_recode_w(W, NW, x.v, [&](int i, int d) { a[i] = d; });
    sc_recode_fixed<W, NW>(x.v, [&](int i, int d) { b[i] = d; });
    for (int i = 0; i < NW; i++) {
        if (a[i] != b[i] || b[i] < -(1 << (W - 1)) || b[i] > (1 << (W - 1))) {
            fprintf(stderr, "recode W=%d NW=%d %s: window %d is %d, sc_recode_w gives %d\n", W, NW, what, i, b[i], a[i]);
            return false;
        }
    }
    g_checks++;
    return true;
}

template <int W, int NW>
static bool recode_geometry() {
    const U256 one = u_pow2(0);
    std::vector<U256> xs;
    xs.push_back(u_zero());
    xs.push_back(one);
    { U256 l; memcpy(l.v, SC_L, sizeof l.v); xs.push_back(u_sub(l, one)); }
    const int k = 252 / W;                           // whole windows below l
    // a carry through every whole window: half in window 0, half - 1 above it
    U256 allneg = u_pow2(W - 1), allpos = u_zero();
    for (int i = 0; i < k; i++) {
        U256 d = u_sub(u_pow2(W * i + W - 1), u_pow2(W * i));       // (half - 1) << (W i)
        if (i) allneg = u_add(allneg, d);
        allpos = u_add(allpos, d);
    }
    xs.push_back(allneg);
    xs.push_back(allpos);
    for (int i = 1; i < NW; i++) {
        if (W * i > 252) break;
        const U256 b = u_pow2(W * i);
        xs.push_back(u_sub(b, one));                  // all ones below the boundary: a carry into window i
        xs.push_back(b);
        xs.push_back(u_add(b, one));
        xs.push_back(u_add(u_sub(b, one), u_pow2(W * i + W - 1)));   // ... into a window that holds half already
        if (i < k) {
            xs.push_back(u_add(allneg, b));           // the chain with window i one higher (still carries on)
            xs.push_back(u_sub(allneg, b));           // ... and one lower (the chain ends here)
            xs.push_back(u_sub(allneg, u_pow2(W * i - 1)));
        }
    }
    for (auto& x : xs) {
        if (!u_below_l(x)) continue;
        if (!recode_same<W, NW>(x, "edge")) return false;
    }
    for (int t = 0; t < 20000; t++) {
        sc r; U256 x;
        rnd_sc(r);
        sc_from_mont(x.v, r);
        if (!recode_same<W, NW>(x, "random")) return false;
    }
    return true;
}

static bool shared_fold_scalars() {
    const int N = 32, lgN = 5;
    for (int trial = 0; trial < 8; trial++) {
        sc y, yinv, u[5], ui[5];
        rnd_sc(y);
        sc_invert_vartime_mont(yinv, y);
        for (int t = 0; t < 5; t++) { rnd_sc(u[t]); sc_invert_vartime_mont(ui[t], u[t]); }
        sc yi_m[N], yi_p[N];                           // y^-j in Montgomery and in plain form (RangeArgs::s2 holds the latter)
        for (int j = 0; j < N; j++) { sc_pow_mont(yi_m[j], yinv, (uint32_t)j); sc_from_mont(yi_p[j].v, yi_m[j]); }
        std::vector<sc> TH(1);
        sc_one_mont(TH[0]);
        for (int r = 1; r <= 4; r++) {                 // TH_r from TH_(r-1), as k_rp_fold extends it: TH'[2t + bit] = TH[t] * (bit ? u^-1 : u)
            std::vector<sc> nx(TH.size() * 2);
            for (size_t t = 0; t < TH.size(); t++)
                for (int bit = 0; bit < 2; bit++) sc_montmul(nx[2 * t + bit], TH[t], bit ? ui[r - 1] : u[r - 1]);
            TH = nx;
            const int T = N >> r;
            for (int j = 0; j < N; j++) {
                const int i = j & (T - 1), k = j >> (lgN - r);
                sc want, ck, got;
                sc_montmul(want, yi_p[j], TH[j >> (lgN - r)]);          // coeff_plain: plain x Montgomery = plain
                sc_montmul(ck, yi_p[k * T], TH[k]);                     // the shared scalar of (H side, k), plain
                sc_montmul(got, ck, yi_m[i]);                           // ... times y^-i
                if (memcmp(got.v, want.v, sizeof got.v) != 0) {
                    fprintf(stderr, "shared fold scalars: trial %d, %d rounds, generator %d = %d + %d * %d differs\n", trial, r, j, i, k, T);
                    return false;
                }
                g_checks++;
            }
        }
    }
    return true;
}

int main() {
    bool ok = recode_geometry<17, 15>() && recode_geometry<16, 16>() && recode_geometry<11, 24>() && recode_geometry<5, 51>();
    ok = ok && shared_fold_scalars();
    if (!ok) return 1;
    printf("ok %ld\n", g_checks);
    return 0;
}
