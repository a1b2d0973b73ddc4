// DEFLATE and CRC-32 of a device buffer, so that .npz members and .nii.gz files can be compressed where their arrays are made and only the
// compressed bytes cross to the host (cineflow/deflate.py builds the zip and gzip containers around them).
//   * cf_deflate: the input is cut into chunks of CH = 32768 bytes; one workgroup compresses one chunk into a fixed slot (deflate_core.h:
//     hash heads and the chunk in LDS, longest match per position, an exact greedy parse, dynamic Huffman codes limited to 15 / 7 bits, bits
//     OR-ed into zeroed LDS words; a stored block when that is not smaller), chunks never reference each other and each ends on a byte
//     boundary as a non-final block, the way pigz writes them.  A one-workgroup scan of the slot sizes (select_scan_kernel's shape in
//     dataset.hip) and a gather make the stream contiguous.  The parse is the three-walk form of deflate_core.h and not pointer doubling:
//     doubling needs two 64 KiB jump tables beside the chunk, more than a CU's 160 KiB of LDS, and its 15 rounds over 32768 positions cost
//     more than the 256 + 128 + 256 dependent LDS steps of the walks.
//   * cf_crc32 is a kernel of its own and not folded into cf_deflate: the .nii.gz route checksums a header the device never sees, callers
//     checksum without compressing (numpy arrays that go through zlib), and it is tested on its own against zlib.  Every thread runs the
//     bytewise table over 1 KiB, a workgroup folds its 256 partials in a tree with the "append 2^k KiB of zeros" operators (a GF(2)
//     polynomial product mod P, deflate_core.h), a second launch folds the workgroups' partials the same way.  The pieces are aligned to
//     the END of the buffer: zero bytes in FRONT of a message leave a CRC register that starts at 0 untouched, so the short piece is the
//     first one and every operator is a fixed power; the effect of the 0xFFFFFFFF start value is one more operator, applied on the host.
// Integer and LDS work only; 143 KiB of LDS per workgroup, one workgroup per CU (a 5.5 MB case is 170 chunks on 256 CUs).
// The same bytes on every run: see deflate_core.h.
#include "common.h"
#include "deflate_core.h"

namespace cf {

using namespace dfl;

constexpr int DF_THREADS = 256;
constexpr int DF_GRID_MAX = 512;                        // workgroups of the compress kernel (each owns CH uint32 of match state in ws)
constexpr int CRC_PIECE = 1024, CRC_THREADS = 256;
constexpr long CRC_WG_BYTES = (long)CRC_PIECE * CRC_THREADS;

struct DevX {
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int nt() const { return DF_THREADS; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void amax(int* a, int v) const { atomicMax(a, v); }
    __device__ __forceinline__ void aadd(uint32_t* a, uint32_t v) const { atomicAdd(a, v); }
    __device__ __forceinline__ void aor(uint32_t* a, uint32_t v) const { atomicOr(a, v); }
};

constexpr size_t DF_LDS_BUF = CH + BUF_PAD, DF_LDS_STEP = CH, DF_LDS_BIG = 2 * CH;
constexpr size_t DF_LDS = DF_LDS_BUF + DF_LDS_STEP + DF_LDS_BIG + ((sizeof(Small) + 15) & ~(size_t)15);
static_assert(DF_LDS <= 160 * 1024, "one chunk's state must fit a CU's LDS");
static_assert(CH % DF_THREADS == 0 && SLAB % DF_THREADS == 0, "ranges and slabs are whole per thread");

__global__ void __launch_bounds__(DF_THREADS) deflate_chunks_kernel(const uint8_t* __restrict__ src, long n, int nchunks, uint32_t* __restrict__ mws,
                                                                    uint8_t* __restrict__ slots, int* __restrict__ sizes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    State st;
    st.buf = lds;
    st.step = lds + DF_LDS_BUF;
    st.big = reinterpret_cast<uint32_t*>(lds + DF_LDS_BUF + DF_LDS_STEP);
    st.s = reinterpret_cast<Small*>(lds + DF_LDS_BUF + DF_LDS_STEP + DF_LDS_BIG);
    st.m = mws + (long)blockIdx.x * CH;
    DevX x;
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long off = (long)c * CH;
        const int len = n - off < CH ? (int)(n - off) : CH;
        compress_chunk(x, src + off, len, st, slots + (long)c * SLOT, sizes + c);
    }
}

// one workgroup: sizes -> exclusive offsets, *total = the stream's length
__global__ void __launch_bounds__(256) deflate_scan_kernel(const int* __restrict__ sizes, int nchunks, long long* __restrict__ offsets,
                                                           long long* __restrict__ total) {
    __shared__ long long ws[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int base = 0; base < nchunks; base += 256) {
        const int i = base + threadIdx.x;
        const long long c = i < nchunks ? sizes[i] : 0;
        long long incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += ws[w];
            all += ws[w];
        }
        if (i < nchunks) offsets[i] = carry + before + incl - c;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// one workgroup per chunk: its slot to its place in the stream.  The place has any alignment: the head and tail go bytewise, the middle as
// aligned words put together from the slot's bytes.
__global__ void __launch_bounds__(256) deflate_gather_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ sizes,
                                                             const long long* __restrict__ offsets, uint8_t* __restrict__ out) {
    const int c = blockIdx.x, size = sizes[c];
    const uint8_t* s = slots + (long)c * SLOT;
    uint8_t* d = out + offsets[c];
    int head = (int)((4 - (reinterpret_cast<uintptr_t>(d) & 3)) & 3);
    if (head > size) head = size;
    const int words = (size - head) / 4;
    if ((int)threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    uint32_t* dw = reinterpret_cast<uint32_t*>(d + head);
    for (int i = threadIdx.x; i < words; i += 256) {
        const uint8_t* q = s + head + 4 * i;
        dw[i] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
    const int done = head + 4 * words;
    if ((int)threadIdx.x < size - done) d[done + threadIdx.x] = s[done + threadIdx.x];
}

// build_lengths on its own, for a histogram the caller brings: the length limit has a test that does not depend on what a match finder
// leaves of a fixture's byte counts
__global__ void __launch_bounds__(DF_THREADS) code_lengths_kernel(const uint32_t* __restrict__ freq, int n, int maxbits, uint8_t* __restrict__ lens) {
    __shared__ Small s;
    __shared__ uint32_t f[288];
    __shared__ uint8_t l[288];
    for (int i = threadIdx.x; i < 288; i += DF_THREADS) f[i] = i < n ? freq[i] : 0u;
    __syncthreads();
    DevX x;
    build_lengths(x, s, f, n, maxbits, l);
    for (int i = threadIdx.x; i < n; i += DF_THREADS) lens[i] = l[i];
}

struct CrcOps { uint32_t x[8]; };

// a workgroup's 256 partials -> one, by a tree: at level k the right neighbour absorbs the left one shifted by 2^k pieces
__device__ __forceinline__ uint32_t crc_fold256(uint32_t c, uint32_t* sh, const CrcOps& ops) {
    const int t = threadIdx.x;
    sh[t] = c;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = 1 << k;
        if ((t & (2 * s - 1)) == 2 * s - 1) sh[t] = gf_mul(ops.x[k], sh[t - s]) ^ sh[t];
        __syncthreads();
    }
    return sh[255];
}

// part[w] = the CRC register (start 0, no final xor) after the 256 KiB that end at byte n - (nwg - 1 - w) 256 KiB; bytes before 0 are zeros
__global__ void __launch_bounds__(CRC_THREADS) crc_pieces_kernel(const uint8_t* __restrict__ src, long n, long pad, CrcOps ops,
                                                                 uint32_t* __restrict__ part) {
    __shared__ uint32_t table[256], sh[CRC_THREADS];
    table[threadIdx.x] = crc_table_entry(threadIdx.x);
    __syncthreads();
    const long g = (long)blockIdx.x * CRC_THREADS + threadIdx.x;
    long lo = g * CRC_PIECE - pad;
    const long hi = lo + CRC_PIECE;
    if (lo < 0) lo = 0;
    uint32_t c = 0;
    for (long i = lo; i < hi; ++i) c = table[(c ^ src[i]) & 0xFF] ^ (c >> 8);
    c = crc_fold256(c, sh, ops);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}

// one workgroup: thread t folds R consecutive partials (aligned to the end again), the tree folds the threads; fin = the start value's
// contribution and the final xor
__global__ void __launch_bounds__(CRC_THREADS) crc_fold_kernel(const uint32_t* __restrict__ part, int nwg, int R, uint32_t xw, CrcOps ops,
                                                               uint32_t fin, uint32_t* __restrict__ crc) {
    __shared__ uint32_t sh[CRC_THREADS];
    const long padw = (long)R * CRC_THREADS - nwg;
    uint32_t c = 0;
    for (int r = 0; r < R; ++r) {
        const long i = (long)threadIdx.x * R + r - padw;
        c = gf_mul(xw, c) ^ (i >= 0 ? part[i] : 0u);
    }
    c = crc_fold256(c, sh, ops);
    if (threadIdx.x == 0) *crc = c ^ fin;
}

static inline long deflate_chunks(long n) { return (n + CH - 1) / CH; }
static inline long round256(long v) { return (v + 255) & ~255L; }

}  // namespace cf

using namespace cf;

extern "C" int cf_deflate_chunk_bytes(void) { return CH; }

extern "C" long cf_deflate_bound(long n) { return n < 0 ? CF_ERR_ARG : n + 5 * deflate_chunks(n); }

extern "C" long cf_deflate_workspace_bytes(long n) {
    if (n < 0) return CF_ERR_ARG;
    const long nc = deflate_chunks(n), grid = nc < DF_GRID_MAX ? nc : DF_GRID_MAX;
    return 256 + round256(4 * nc) + round256(8 * nc) + grid * CH * 4 + nc * SLOT;
}

extern "C" int cf_deflate(const void* src, long n, void* out, long out_cap, void* ws, long ws_bytes, long long* out_bytes_dev, void* stream) {
    CF_REQUIRE(n >= 0, "n = %ld is negative", n);
    CF_REQUIRE(src && out && ws && out_bytes_dev, "null pointer");
    CF_REQUIRE(out_cap >= cf_deflate_bound(n), "out_cap = %ld is below cf_deflate_bound(%ld) = %ld", out_cap, n, cf_deflate_bound(n));
    CF_REQUIRE(ws_bytes >= cf_deflate_workspace_bytes(n), "workspace of %ld bytes is below cf_deflate_workspace_bytes(%ld) = %ld", ws_bytes, n,
               cf_deflate_workspace_bytes(n));
    CF_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "the workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(out_bytes_dev, 0, sizeof(long long), st) != hipSuccess) { set_error(std::string(__func__) + ": memset failed"); return CF_ERR_LAUNCH; }
        return CF_OK;
    }
    const long nc = deflate_chunks(n);
    CF_REQUIRE(nc < (1L << 31), "n = %ld bytes is more than 2^31 chunks", n);
    const int grid = (int)(nc < DF_GRID_MAX ? nc : DF_GRID_MAX);
    unsigned char* w = static_cast<unsigned char*>(ws);
    int* sizes = reinterpret_cast<int*>(w + 256);
    long long* offsets = reinterpret_cast<long long*>(w + 256 + round256(4 * nc));
    uint32_t* mws = reinterpret_cast<uint32_t*>(w + 256 + round256(4 * nc) + round256(8 * nc));
    uint8_t* slots = reinterpret_cast<uint8_t*>(mws) + (long)grid * CH * 4;
    // (asked on every call: the attribute is per device, and a flag kept here would be shared by the threads that call this)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(deflate_chunks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DF_LDS);
    if (e != hipSuccess) {
        set_error(std::string(__func__) + ": the device refused " + std::to_string(DF_LDS) + " bytes of LDS per workgroup: " + hipGetErrorString(e));
        return CF_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(deflate_chunks_kernel, dim3(grid), dim3(DF_THREADS), DF_LDS, st, static_cast<const uint8_t*>(src), n, (int)nc, mws, slots, sizes);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(256), 0, st, sizes, (int)nc, offsets, out_bytes_dev);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(deflate_gather_kernel, dim3((int)nc), dim3(256), 0, st, slots, sizes, offsets, static_cast<uint8_t*>(out));
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" int cf_huffman_code_lengths(const unsigned* freq, int n, int max_bits, unsigned char* lens, void* stream) {
    CF_REQUIRE(freq && lens, "null pointer");
    CF_REQUIRE(n >= 2 && n <= NLL, "n = %d symbols is outside 2..%d", n, NLL);
    CF_REQUIRE(max_bits >= 1 && max_bits <= 15 && (1 << max_bits) >= n, "max_bits = %d cannot hold %d symbols (1..15 bits)", max_bits, n);
    hipLaunchKernelGGL(code_lengths_kernel, dim3(1), dim3(DF_THREADS), 0, as_stream(stream), freq, n, max_bits, lens);
    CF_CHECK_LAUNCH();
    return CF_OK;
}

extern "C" long cf_crc32_workspace_bytes(long n) { return n < 0 ? CF_ERR_ARG : 256 + 4 * ((n + CRC_WG_BYTES - 1) / CRC_WG_BYTES); }

extern "C" int cf_crc32(const void* src, long n, void* ws, long ws_bytes, unsigned* crc_dev, void* stream) {
    CF_REQUIRE(n >= 0, "n = %ld is negative", n);
    CF_REQUIRE(src && ws && crc_dev, "null pointer");
    CF_REQUIRE(ws_bytes >= cf_crc32_workspace_bytes(n), "workspace of %ld bytes is below cf_crc32_workspace_bytes(%ld) = %ld", ws_bytes, n,
               cf_crc32_workspace_bytes(n));
    CF_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "the workspace must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(crc_dev, 0, sizeof(unsigned), st) != hipSuccess) { set_error(std::string(__func__) + ": memset failed"); return CF_ERR_LAUNCH; }
        return CF_OK;
    }
    const long nwg = (n + CRC_WG_BYTES - 1) / CRC_WG_BYTES;
    CF_REQUIRE(nwg < (1L << 31), "n = %ld bytes is too long", n);
    const int R = (int)((nwg + CRC_THREADS - 1) / CRC_THREADS);
    CrcOps piece_ops, fold_ops;                    // sixteen small powers, computed per call: nothing is shared between calling threads
    for (int k = 0; k < 8; ++k) piece_ops.x[k] = gf_xpow8((uint64_t)CRC_PIECE << k);
    for (int k = 0; k < 8; ++k) fold_ops.x[k] = gf_xpow8(((uint64_t)CRC_WG_BYTES * (uint64_t)R) << k);
    const uint32_t fin = gf_mul(gf_xpow8((uint64_t)n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    uint32_t* part = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(ws));
    hipLaunchKernelGGL(crc_pieces_kernel, dim3((int)nwg), dim3(CRC_THREADS), 0, st, static_cast<const uint8_t*>(src), n, nwg * CRC_WG_BYTES - n, piece_ops,
                       part);
    CF_CHECK_LAUNCH();
    hipLaunchKernelGGL(crc_fold_kernel, dim3(1), dim3(CRC_THREADS), 0, st, part, (int)nwg, R, gf_xpow8((uint64_t)CRC_WG_BYTES), fold_ops, fin, crc_dev);
    CF_CHECK_LAUNCH();
    return CF_OK;
}
