// seq_kernels.hip -- gfx950 kernels that turn a resident sequence into the arrays the seed stage reads: code bytes, 4-bit
// class codes, 2-bit codes + special masks with the byte-presence flags, and the half-overlapping 64-byte blocks of the
// target's arrays.  (DESIGN.md section 2 lays these arrays out; they are the inputs of every row of section 3's table.)
#include <hip/hip_runtime.h>
#include "lz_ctx.hpp"
#include "lz_lut.hpp"
#include "lz_seed_dev.hpp"

// ------------------------------------------------------------------------------------------
// byte -> code translation (one pass per sequence; the table folds charToBits and the score
// class of the byte, see lz_common.hpp)
__global__ void __launch_bounds__(LZ_TPB)
k_encode(const u8* __restrict__ raw, u8* __restrict__ code, u32 len, const u8* __restrict__ cls)
{
    __shared__ u8 tab[256];
    tab[threadIdx.x] = cls[threadIdx.x];
    __syncthreads();
    const u32 nvec = (len + 15u) >> 4;                 // buffers are padded: whole 16-byte groups are safe
    for (u32 v = blockIdx.x * LZ_TPB + threadIdx.x; v < nvec; v += gridDim.x * LZ_TPB) {
        uint4 x = reinterpret_cast<const uint4*>(raw)[v];
        u32 w[4] = { x.x, x.y, x.z, x.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u32 a = w[k];
            w[k] = (u32)tab[a & 255u] | ((u32)tab[(a >> 8) & 255u] << 8) |
                   ((u32)tab[(a >> 16) & 255u] << 16) | ((u32)tab[a >> 24] << 24);
        }
        reinterpret_cast<uint4*>(code)[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// 4-bit class codes for phase A: nib[b] = class(code[2b]) | class(code[2b+1]) << 4, over the whole padded
// code array (padding bytes carry class 0 there and here)
__global__ void __launch_bounds__(LZ_TPB)
k_pack_nibbles(const u8* __restrict__ code, u8* __restrict__ nib, size_t nbytes)
{
    const size_t b = (size_t)blockIdx.x * LZ_TPB + threadIdx.x;
    if (b < nbytes) nib[b] = (u8)((code[2 * b] & 7u) | ((code[2 * b + 1] & 7u) << 4));
}
int lzk_pack_nibbles(LzCtx& c, const u8* code_alloc, u8* nib, size_t nbytes)
{
    hipLaunchKernelGGL(k_pack_nibbles, dim3((unsigned)((nbytes + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream, code_alloc, nib, nbytes);
    LZ_HIP(hipGetLastError());
    return 0;
}

int lzk_encode(LzCtx& c, const u8* raw, u8* code, u32 len, const u8* cls256_dev, hipStream_t st, KernelTimer* timer)
{
    if (len == 0) return 0;
    if (!st) st = c.stream;
    if (!timer) timer = &c.timer;
    u32 nvec = (len + 15u) >> 4;
    u32 blocks = (nvec + LZ_TPB - 1) / LZ_TPB; if (blocks > 4096) blocks = 4096;
    timer->begin("k_encode", st);
    hipLaunchKernelGGL(k_encode, dim3(blocks), dim3(LZ_TPB), 0, st, raw, code, len, cls256_dev);
    timer->end(st);
    LZ_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// 2-bit codes + special masks for phase A (lz_lut.hpp), from the code bytes: one thread per mask byte (8 bases).
// Base i of the sequence is bit (i + LZ_PAD2); bases outside [-LZ_SEQ_PAD, len + LZ_SEQ_PAD) are padding: special.
__global__ void __launch_bounds__(LZ_TPB)
k_pack2(const u8* __restrict__ code /*base 0*/, u32 len, u8* __restrict__ two, u8* __restrict__ spc, u32 nmask)
{
    const u32 j = blockIdx.x * LZ_TPB + threadIdx.x;
    if (j >= nmask) return;
    u32 bits = 0, m = 0;
    const s64 b0 = (s64)j * 8 - LZ_PAD2;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const s64 i = b0 + k;
        const u32 c = (i >= -(s64)LZ_SEQ_PAD && i < (s64)len + LZ_SEQ_PAD) ? code[i] : (u32)LZ_CODE_INVALID;
        if (c & LZ_CODE_INVALID) m |= 1u << k; else bits |= LZ_GRAY(LZ_CODE_BITS(c)) << (2 * k);
    }
    spc[j] = (u8)m;
    two[2 * (size_t)j] = (u8)bits; two[2 * (size_t)j + 1] = (u8)(bits >> 8);
}
// which byte values occur in raw[0..len): flags[b] != 0
__global__ void __launch_bounds__(LZ_TPB)
k_byte_presence(const u8* __restrict__ raw, u32 len, u32* __restrict__ flags)
{
    __shared__ u32 f[256];
    f[threadIdx.x] = 0;
    __syncthreads();
    const u32 nvec = (len + 15u) >> 4;                 // padded buffers: whole 16-byte groups are readable (padding is 0)
    for (u32 v = blockIdx.x * LZ_TPB + threadIdx.x; v < nvec; v += gridDim.x * LZ_TPB) {
        const uint4 x = reinterpret_cast<const uint4*>(raw)[v];
        const u32 w[4] = { x.x, x.y, x.z, x.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u32 a = w[k];
            if ((size_t)v * 16 + 4 * k + 0 < len) f[a & 255u] = 1;
            if ((size_t)v * 16 + 4 * k + 1 < len) f[(a >> 8) & 255u] = 1;
            if ((size_t)v * 16 + 4 * k + 2 < len) f[(a >> 16) & 255u] = 1;
            if ((size_t)v * 16 + 4 * k + 3 < len) f[a >> 24] = 1;
        }
    }
    __syncthreads();
    if (f[threadIdx.x]) flags[threadIdx.x] = 1;
}
// Block k of dst = bytes [32k, 32k + 64) of src: every run of up to 32 bytes of src lies inside ONE 64-byte line of
// dst (the block its first byte's 32-byte half starts).  Phase A reads 31-32 consecutive bytes of the target's 2-bit
// array around every hit, at a random place: from the plain array that is 1.5 cache lines per hit on average, and the
// scan kernel runs exactly as fast as its CU's L1 can have lines in flight (64 x 64 B per ~460 cycles).
__global__ void __launch_bounds__(LZ_TPB)
k_overlap32(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t nchunks)
{
    const size_t v = (size_t)blockIdx.x * LZ_TPB + threadIdx.x;           // 16-byte chunk of dst: block v / 4, quarter v % 4
    if (v < nchunks) dst[v] = src[2 * (v >> 2) + (v & 3u)];
}
int lzk_overlap32(LzCtx& c, const u8* src, u8* dst, size_t nblocks)
{
    const size_t nchunks = nblocks * 4;
    hipLaunchKernelGGL(k_overlap32, dim3((unsigned)((nchunks + LZ_TPB - 1) / LZ_TPB)), dim3(LZ_TPB), 0, c.stream,
                       reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), nchunks);
    LZ_HIP(hipGetLastError());
    return 0;
}

int lzk_pack2(LzCtx& c, const u8* code_base, const u8* raw_base, u32 len, u8* two, u8* spc, u32 nmask, u32* flags256)
{
    LZ_HIP(hipMemsetAsync(flags256, 0, 256 * 4, c.stream));
    c.timer.begin("k_pack2", c.stream);
    hipLaunchKernelGGL(k_pack2, dim3((nmask + LZ_TPB - 1) / LZ_TPB), dim3(LZ_TPB), 0, c.stream, code_base, len, two, spc, nmask);
    c.timer.end(c.stream);
    if (len) {
        u32 blocks = (((len + 15u) >> 4) + LZ_TPB - 1) / LZ_TPB; if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(k_byte_presence, dim3(blocks), dim3(LZ_TPB), 0, c.stream, raw_base, len, flags256);
    }
    LZ_HIP(hipGetLastError());
    return 0;
}
