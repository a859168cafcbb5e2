// Test-only device program: the PRODUCT headers (dapol_amd/csrc/{ge,sc,hash,ge_quad}.h) as the GPU compiles them -- the
// v_mad chains of fe_mul / fe_sq, sc_mad, the four-lanes-per-point formulas and the wavefront-held STROBE -- one case per
// lane (or per quad, or per wavefront), on the operands of tests/limb_vectors.py.  Built by tests/test_gpu_device_arith.py
// with the library's own flags into tests/_build/; never linked into libdapol_hip.so.
//
// Every extern "C" wrapper copies its inputs in, launches once, copies the outputs out and returns the first hipError_t it
// saw (0 = hipSuccess).  Every kernel checks its case index against n; the quad and STROBE kernels need whole wavefronts, so
// their wrappers pad the launch and the kernels clamp the case they READ and skip the write.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "../dapol_amd/csrc/ge.h"
#include "../dapol_amd/csrc/sc.h"
#include "../dapol_amd/csrc/hash.h"
#include "../dapol_amd/csrc/ge_quad.h"
#include "arith_cases.h"
using namespace dapol;
using namespace dapol_test;

enum { BLOCK = 64 };

// ---------------------------------------------------------------------------------------------- one case per lane
__global__ void k_fe_cases(int op, int n, const int32_t* f, const int32_t* g, int32_t* ol, uint32_t* ow, int32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flags[i] = fe_case(op, f + 9 * i, g + 9 * i, ol + 9 * i, ow + 8 * i);
}
__global__ void k_ge_cases(int op, int n, const int32_t* p, const int32_t* q, const int32_t* neg, int32_t* ol, uint32_t* ow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ge_case(op, p + 36 * i, q + 36 * i, neg[i], ol + 36 * i, ow + 8 * i);
}
__global__ void k_ge_decompress_cases(int n, const uint32_t* in, int32_t* ok, int32_t* ol, uint32_t* ow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ok[i] = ge_decompress_case(in + 8 * i, ol + 36 * i, ow + 8 * i);
}
__global__ void k_ge_uniform_cases(int n, const uint32_t* in, int32_t* ol, uint32_t* ow) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ge_uniform_case(in + 16 * i, ol + 36 * i, ow + 8 * i);
}
__global__ void k_sc_cases(int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc_case(op, a + 8 * i, b + 8 * i, out + 8 * i);
}
__global__ void k_sc_wide_cases(int n, const uint32_t* w, uint32_t* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc_wide_case(w + 16 * i, out + 8 * i);
}
__global__ void k_sc_recode_cases(int n, const int32_t* wn, const uint32_t* x, int32_t* digits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sc_recode_case(wn[2 * i], wn[2 * i + 1], x + 8 * i, digits + RECODE_MAX_NW * i);
}

// ---------------------------------------------------------------------------------------------- one point per four lanes
// Lane 4 g + k of the launch holds coordinate k of case g's point p (ge_quad.h).  Whole 64-lane wavefronts only: a case index
// past n reads case n - 1 again and writes nothing.  op as in arith_cases.h (GEOP_NEG has no quad form).
__global__ void k_quad_cases(int op, int n, const int32_t* p, const int32_t* q, const int32_t* neg, int32_t* ol) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, grp = t >> 2, ql = t & 3;
    const int i = grp < n ? grp : n - 1;
    const bool ng = neg[i] != 0;
    fe c, d;
    fe_load(c, p + 36 * i + 9 * ql);
    fe_load(d, q + 36 * i + 9 * ql);
    // the niels entry of q as quad_madd wants it: lane 0 y-x (y+x if neg), lane 1 y+x (y-x if neg), lane 3 2dxy
    ge_p3 qq;
    ge_load(qq, q + 36 * i);
    ge_niels nl;
    ge_to_niels(nl, qq.X, qq.Y);
    fe qel;
    for (int k = 0; k < FE_NL; k++) qel.v[k] = ql == 0 ? (ng ? nl.ypx.v[k] : nl.ymx.v[k]) : ql == 1 ? (ng ? nl.ymx.v[k] : nl.ypx.v[k]) : nl.xy2d.v[k];
    switch (op) {                                                // (uniform across the launch: every lane stays active)
        case GEOP_MADD: quad_madd(c, ql, qel, ng); break;
        case GEOP_ADD: quad_add(c, ql, d); break;
        case GEOP_DBL: quad_dbl(c, ql); break;
        case GEOP_ADD_CACHED: {
            fe qc;
            quad_to_cached(qc, d, ql);
            quad_add_cached(c, ql, qc, ng);
            break;
        }
        default:                                                 // GEOP_CHAIN
            for (int k = 0; k < GE_CHAIN_ROUNDS; k++) {
                quad_madd(c, ql, qel, ng);
                for (int j = 0; j < GE_CHAIN_DBLS; j++) quad_dbl(c, ql);
            }
            break;
    }
    if (grp < n) fe_store(ol + 36 * grp + 9 * ql, c);
}

// ---------------------------------------------------------------------------------------------- wavefront STROBE
// One block of two wavefronts per case: wavefront 0 replays the transcript in a WStrobe (all 64 lanes in step), lane 0 of
// wavefront 1 replays it in the one-lane Strobe.  Transcript: init, append(filler: k bytes), append_words(n words),
// challenge, append_words(the same words reversed), challenge.  out: [case][2 holders][32 words]; pos: [case][2] = the
// in-block position of the first message word.
__global__ void k_strobe_cases(int ncase, const int32_t* kn, const char* filler, const uint32_t* words, const uint32_t* words_rev, uint32_t* out,
                               uint32_t* pos) {
    const int cs = blockIdx.x < (unsigned)ncase ? (int)blockIdx.x : ncase - 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = kn[2 * cs], nw = kn[2 * cs + 1];
    uint32_t o[32];
    if (wave == 0) {
        WStrobe st;
        wstrobe_lanes(st, lane);
        const uint32_t at = strobe_replay(st, filler, k, words, words_rev, nw, o,
                                   [](WStrobe& s, const uint32_t* w, int n) { for (int i = 0; i < n; i++) strobe_absorb_word(s, w[i]); });
        if (lane == 0 && blockIdx.x < (unsigned)ncase) {
            for (int i = 0; i < 32; i++) out[64 * cs + i] = o[i];
            pos[2 * cs] = at;
        }
    } else if (lane == 0) {
        Strobe st;
        const uint32_t at = strobe_replay(st, filler, k, words, words_rev, nw, o, [](Strobe& s, const uint32_t* w, int n) {
            for (int i = 0; i < n; i++)
                for (int b = 0; b < 4; b++) strobe_absorb_byte(s, (uint8_t)(w[i] >> (8 * b)));
        });
        if (blockIdx.x < (unsigned)ncase) {
            for (int i = 0; i < 32; i++) out[64 * cs + 32 + i] = o[i];
            pos[2 * cs + 1] = at;
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side
namespace {
struct Run {                                                     // device buffers of one wrapper call; the first error sticks
    hipError_t err = hipSuccess;
    std::vector<void*> bufs;
    void note(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; }
    template <class T>
    T* in(const T* host, size_t count) {
        T* d = out<T>(count);
        if (d && count) note(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <class T>
    T* out(size_t count) {
        void* d = nullptr;
        if (err != hipSuccess) return nullptr;
        note(hipMalloc(&d, (count ? count : 1) * sizeof(T)));
        if (d) { bufs.push_back(d); note(hipMemset(d, 0, (count ? count : 1) * sizeof(T))); }
        return (T*)d;
    }
    template <class T>
    void back(T* host, const T* dev, size_t count) {
        if (err == hipSuccess && count) note(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
    }
    bool ok() const { return err == hipSuccess; }
    void launched() { note(hipGetLastError()); note(hipDeviceSynchronize()); }
    int done() {
        for (void* b : bufs) note(hipFree(b));
        return (int)err;
    }
};
dim3 grid_for(int n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }
}  // namespace

extern "C" {
int d_fe_cases(int op, int n, const int32_t* f, const int32_t* g, int32_t* out_limbs, uint32_t* out_words, int32_t* flags) {
    if (n <= 0) return 0;
    Run r;
    const size_t N = (size_t)n;
    const int32_t *df = r.in(f, 9 * N), *dg = r.in(g, 9 * N);
    int32_t *dl = r.out<int32_t>(9 * N), *dfl = r.out<int32_t>(N);
    uint32_t* dw = r.out<uint32_t>(8 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_fe_cases, grid_for(n), dim3(BLOCK), 0, 0, op, n, df, dg, dl, dw, dfl); r.launched(); }
    r.back(out_limbs, dl, 9 * N); r.back(out_words, dw, 8 * N); r.back(flags, dfl, N);
    return r.done();
}
int d_ge_cases(int op, int n, const int32_t* p, const int32_t* q, const int32_t* neg, int32_t* out_limbs, uint32_t* out_words) {
    if (n <= 0) return 0;
    Run r;
    const size_t N = (size_t)n;
    const int32_t *dp = r.in(p, 36 * N), *dq = r.in(q, 36 * N), *dn = r.in(neg, N);
    int32_t* dl = r.out<int32_t>(36 * N);
    uint32_t* dw = r.out<uint32_t>(8 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_ge_cases, grid_for(n), dim3(BLOCK), 0, 0, op, n, dp, dq, dn, dl, dw); r.launched(); }
    r.back(out_limbs, dl, 36 * N); r.back(out_words, dw, 8 * N);
    return r.done();
}
int d_ge_decompress_cases(int n, const uint32_t* in, int32_t* ok, int32_t* out_limbs, uint32_t* out_words) {
    if (n <= 0) return 0;
    Run r;
    const size_t N = (size_t)n;
    const uint32_t* di = r.in(in, 8 * N);
    int32_t *dok = r.out<int32_t>(N), *dl = r.out<int32_t>(36 * N);
    uint32_t* dw = r.out<uint32_t>(8 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_ge_decompress_cases, grid_for(n), dim3(BLOCK), 0, 0, n, di, dok, dl, dw); r.launched(); }
    r.back(ok, dok, N); r.back(out_limbs, dl, 36 * N); r.back(out_words, dw, 8 * N);
    return r.done();
}
int d_ge_uniform_cases(int n, const uint32_t* in, int32_t* out_limbs, uint32_t* out_words) {
    if (n <= 0) return 0;
    Run r;
    const size_t N = (size_t)n;
    const uint32_t* di = r.in(in, 16 * N);
    int32_t* dl = r.out<int32_t>(36 * N);
    uint32_t* dw = r.out<uint32_t>(8 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_ge_uniform_cases, grid_for(n), dim3(BLOCK), 0, 0, n, di, dl, dw); r.launched(); }
    r.back(out_limbs, dl, 36 * N); r.back(out_words, dw, 8 * N);
    return r.done();
}
int d_sc_cases(int op, int n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    if (n <= 0) return 0;
    Run r;
    const size_t N = (size_t)n;
    const uint32_t *da = r.in(a, 8 * N), *db = r.in(b, 8 * N);
    uint32_t* dout = r.out<uint32_t>(8 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_sc_cases, grid_for(n), dim3(BLOCK), 0, 0, op, n, da, db, dout); r.launched(); }
    r.back(out, dout, 8 * N);
    return r.done();
}
int d_sc_wide_cases(int n, const uint32_t* w, uint32_t* out) {
    if (n <= 0) return 0;
    Run r;
    const size_t N = (size_t)n;
    const uint32_t* dw = r.in(w, 16 * N);
    uint32_t* dout = r.out<uint32_t>(8 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_sc_wide_cases, grid_for(n), dim3(BLOCK), 0, 0, n, dw, dout); r.launched(); }
    r.back(out, dout, 8 * N);
    return r.done();
}
int d_sc_recode_cases(int n, const int32_t* wn, const uint32_t* x, int32_t* digits) {
    if (n <= 0) return 0;
    for (int i = 0; i < n; i++)                                  // the digit rows are RECODE_MAX_NW wide; widths as tables.h allows
        if (wn[2 * i] < WBITS_MIN || wn[2 * i] > WBITS_MAX || wn[2 * i + 1] < 1 || wn[2 * i + 1] > RECODE_MAX_NW) return (int)hipErrorInvalidValue;
    Run r;
    const size_t N = (size_t)n;
    const int32_t* dwn = r.in(wn, 2 * N);
    const uint32_t* dx = r.in(x, 8 * N);
    int32_t* dd = r.out<int32_t>(RECODE_MAX_NW * N);
    if (r.ok()) { hipLaunchKernelGGL(k_sc_recode_cases, grid_for(n), dim3(BLOCK), 0, 0, n, dwn, dx, dd); r.launched(); }
    r.back(digits, dd, RECODE_MAX_NW * N);
    return r.done();
}
// n points, four lanes each, in whole 64-lane wavefronts (16 points per wavefront)
int d_quad_cases(int op, int n, const int32_t* p, const int32_t* q, const int32_t* neg, int32_t* out_limbs) {
    if (n <= 0) return 0;
    if (op == GEOP_NEG) return (int)hipErrorInvalidValue;
    Run r;
    const size_t N = (size_t)n;
    const int32_t *dp = r.in(p, 36 * N), *dq = r.in(q, 36 * N), *dn = r.in(neg, N);
    int32_t* dl = r.out<int32_t>(36 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_quad_cases, dim3((unsigned)((n + 15) / 16)), dim3(BLOCK), 0, 0, op, n, dp, dq, dn, dl); r.launched(); }
    r.back(out_limbs, dl, 36 * N);
    return r.done();
}
// kn: [ncase][2] = (filler bytes k <= filler_len, message words n <= nwords_max); filler, words, words_rev shared by all cases
int d_strobe_cases(int ncase, const int32_t* kn, const char* filler, int filler_len, const uint32_t* words, const uint32_t* words_rev, int nwords_max,
                   uint32_t* out, uint32_t* pos) {
    if (ncase <= 0) return 0;
    for (int i = 0; i < ncase; i++)
        if (kn[2 * i] < 0 || kn[2 * i] > filler_len || kn[2 * i + 1] < 0 || kn[2 * i + 1] > nwords_max) return (int)hipErrorInvalidValue;
    Run r;
    const size_t N = (size_t)ncase;
    const int32_t* dkn = r.in(kn, 2 * N);
    const char* dfill = r.in(filler, (size_t)filler_len);
    const uint32_t *dw = r.in(words, (size_t)nwords_max), *dwr = r.in(words_rev, (size_t)nwords_max);
    uint32_t *dout = r.out<uint32_t>(64 * N), *dpos = r.out<uint32_t>(2 * N);
    if (r.ok()) { hipLaunchKernelGGL(k_strobe_cases, dim3((unsigned)ncase), dim3(2 * BLOCK), 0, 0, ncase, dkn, dfill, dw, dwr, dout, dpos); r.launched(); }
    r.back(out, dout, 64 * N); r.back(pos, dpos, 2 * N);
    return r.done();
}
}
