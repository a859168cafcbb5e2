// The cases of tests/digest_cases.h on the device: SHA-256 / SHA3-256 of dapol_amd/csrc/hash.h as hipcc compiles them for gfx950,
// which is not the host's compilation of the same text.  Same wrappers as tests/digest_host_shim.cpp with the prefix d_; each copies
// its inputs in, launches once, copies the outputs out and returns the first hipError_t it saw (0 = hipSuccess).  Every kernel checks
// its case index against n before it reads or writes.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "digest_cases.h"
using namespace dapol_test;

enum { BLOCK = 64 };

__global__ __launch_bounds__(BLOCK) void k_digest_stream_cases(int kind, int n, uint32_t* out) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n) return;
    uint32_t h[8];
    digest_stream(kind, nullptr, (size_t)l, 0, h);
    for (int i = 0; i < 8; i++) out[8 * l + i] = h[i];
}
__global__ __launch_bounds__(BLOCK) void k_digest_node_cases(int kind, int n, const uint32_t* in, uint32_t* out32, uint32_t* out128) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    uint32_t w[32], a[8], b[8];
    for (int i = 0; i < 32; i++) w[i] = in[32 * c + i];
    digest_nodes(kind, w, a, b);
    for (int i = 0; i < 8; i++) { out32[8 * c + i] = a[i]; out128[8 * c + i] = b[i]; }
}

namespace {
struct Bufs {                        // device buffers of one call, freed on every way out
    void* p[3] = {nullptr, nullptr, nullptr};
    hipError_t err = hipSuccess;
    void* alloc(int k, size_t bytes) {
        if (err == hipSuccess) err = hipMalloc(&p[k], bytes);
        return p[k];
    }
    void step(hipError_t e) { if (err == hipSuccess) err = e; }
    ~Bufs() { for (void* q : p) if (q) (void)hipFree(q); }
};
}  // namespace

extern "C" {
int d_digest_stream_cases(int kind, int n, uint32_t* out /*[n][8]*/) {
    if (n <= 0) return 0;
    Bufs b;
    const size_t bytes = (size_t)n * 32;
    uint32_t* d = (uint32_t*)b.alloc(0, bytes);
    if (b.err == hipSuccess) {
        hipLaunchKernelGGL(k_digest_stream_cases, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, kind, n, d);
        b.step(hipGetLastError());
        b.step(hipDeviceSynchronize());
        b.step(hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
    }
    return (int)b.err;
}
int d_digest_node_cases(int kind, int n, const uint32_t* in /*[n][32]*/, uint32_t* out32 /*[n][8]*/, uint32_t* out128 /*[n][8]*/) {
    if (n <= 0) return 0;
    Bufs b;
    const size_t nin = (size_t)n * 128, nout = (size_t)n * 32;
    uint32_t *di = (uint32_t*)b.alloc(0, nin), *d32 = (uint32_t*)b.alloc(1, nout), *d128 = (uint32_t*)b.alloc(2, nout);
    if (b.err == hipSuccess) {
        b.step(hipMemcpy(di, in, nin, hipMemcpyHostToDevice));
        if (b.err == hipSuccess) {
            hipLaunchKernelGGL(k_digest_node_cases, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, kind, n, di, d32, d128);
            b.step(hipGetLastError());
            b.step(hipDeviceSynchronize());
        }
        b.step(hipMemcpy(out32, d32, nout, hipMemcpyDeviceToHost));
        b.step(hipMemcpy(out128, d128, nout, hipMemcpyDeviceToHost));
    }
    return (int)b.err;
}
}
