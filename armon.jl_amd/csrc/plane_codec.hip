// plane_codec.hip — "xorplane16": the lossless codec of packed checkpoints (no reference counterpart).
//
// A CHUNK encodes one dense plane of R x C elements, row-major, of width W = 64 or 32 bits; u[r][c] is the element's bit
// pattern. Vertical step: t[r][c] = u[r][c] when r % 16 == 0, else u[r][c] ^ u[r-1][c] (row blocks of 16 rows from the chunk's
// first row). A row is cut into G = ceil(C / 64) groups of 64 columns; group g = r G + j, n = R G groups, lane l of group
// (r, j) is column 64 j + l. Horizontal step: base = t[r][64 j], res[0] = 0, res[l] = t[r][64 j + l] ^ t[r][64 j + l - 1] for
// columns inside the plane, 0 past it. mask = the OR of res over the lanes; for every set bit k of mask, ascending, one
// 64-bit word whose bit l is bit k of res[l]. Chunk bytes, little-endian: base[n] (W/8 bytes each, zero-padded to a multiple
// of 8), mask[n] (the same), then the words of group 0, 1, ... back to back.
//
// ONE WAVE PER GROUP, ONE ELEMENT PER LANE: a __ballot over the 64 lanes is one bit-plane of the 64 residuals.
// Encode = masks pass (base, mask and popcount of every group) -> exclusive scan of the popcounts per plane (tiles of 2048,
// three small kernels, no atomics: the layout is a function of the values) -> emit pass (res again, one ballot per set bit,
// lane k keeps plane k and stores it at rank popcount(mask & ((1 << k) - 1)): neighbouring lanes, neighbouring words).
// Decode = popcounts of the mask table -> the same scan -> one wave per (row block, group column) walks its rows: res from
// the words, prefix XOR over the lanes in 6 shuffle steps, XOR with the row above kept in a register; only the requested
// sub-window is written. A group whose words would end past `chunk_bytes` is not read: it sets the status word.
// The scan's words live in the context's reduction scratch (ensure_partials: one synchronisation to grow, refused inside a
// capture); apart from that nothing synchronises with the host. Item numbers are 64-bit, grids 1-D and capped per CU.
#include "common.hpp"

using namespace armon;

namespace {

constexpr int kWave = 64, kWavesPerBlock = kBlock / kWave;
constexpr int kRowBlock = 16;
constexpr int kPerThread = 8, kTile = kBlock * kPerThread;       // elements of the scan per workgroup
constexpr int kMaxPlanes = 8;

template <typename T> struct bits;
template <> struct bits<double> { typedef unsigned long long type; };
template <> struct bits<float> { typedef unsigned int type; };

__host__ __device__ inline uint64_t pad8(uint64_t b) { return (b + 7) & ~7ull; }

__device__ __forceinline__ int popc(unsigned long long v) { return __popcll(v); }
__device__ __forceinline__ int popc(unsigned int v) { return __popc(v); }
__device__ __forceinline__ int lowest(unsigned long long v) { return __ffsll(v) - 1; }
__device__ __forceinline__ int lowest(unsigned int v) { return __ffs(v) - 1; }
// a value every lane holds, as a value the compiler knows to be uniform
// (the builtin returns a signed int: it must not sign-extend into the upper half)
__device__ __forceinline__ unsigned int uniform(unsigned int v) { return (unsigned int)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long uniform(unsigned long long v)
{
    return ((unsigned long long)uniform((unsigned int)(v >> 32)) << 32) | uniform((unsigned int)v);
}

struct shape {
    int64_t R, C, G, n;          // rows, columns, groups per row, groups
    uint64_t table;              // bytes of one table: pad8(n W / 8)
};

// t of the lane's column (0 past the plane) and its residual; called by the whole wave
template <typename U>
__device__ __forceinline__ U residual(const U* __restrict__ plane, const shape& s, int64_t r, int64_t c, int lane, U& t)
{
    t = 0;
    if (c < s.C) {
        t = plane[r * s.C + c];
        if (r % kRowBlock) t ^= plane[(r - 1) * s.C + c];
    }
    const U left = __shfl_up(t, 1, kWave);
    return (lane == 0 || c >= s.C) ? U(0) : U(t ^ left);
}

template <typename U>
struct enc_args {
    const U* dense;              // [nplanes][R][C]
    unsigned char* out;          // chunk of plane q at out + q * capacity
    uint64_t capacity;
    unsigned long long* count;   // [nplanes][n]: popcounts, then their exclusive scan
    shape s;
    int nplanes;
};

template <typename U>
__global__ void __launch_bounds__(kBlock)
k_plane_masks(enc_args<U> a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock, items = a.nplanes * a.s.n;
    for (int64_t item = wave; item < items; item += nwaves) {         // wave-uniform
        const int64_t q = item / a.s.n, g = item % a.s.n, r = g / a.s.G, j = g % a.s.G;
        U t;
        U m = residual(a.dense + q * a.s.R * a.s.C, a.s, r, j * kWave + lane, lane, t);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) m |= __shfl_xor(m, off, kWave);
        if (lane == 0) {
            unsigned char* chunk = a.out + q * a.capacity;
            U* base = reinterpret_cast<U*>(chunk);
            U* mask = reinterpret_cast<U*>(chunk + a.s.table);
            base[g] = t;
            mask[g] = m;
            a.count[item] = (unsigned long long)popc(m);
            if (sizeof(U) == 4 && g == a.s.n - 1 && (a.s.n & 1)) base[a.s.n] = mask[a.s.n] = 0;      // the padding
        }
    }
}

template <typename U>
__global__ void __launch_bounds__(kBlock)
k_plane_emit(enc_args<U> a)
{
    constexpr int W = 8 * sizeof(U);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock, items = a.nplanes * a.s.n;
    for (int64_t item = wave; item < items; item += nwaves) {
        const int64_t q = item / a.s.n, g = item % a.s.n, r = g / a.s.G, j = g % a.s.G;
        unsigned char* chunk = a.out + q * a.capacity;
        const U m = uniform(reinterpret_cast<const U*>(chunk + a.s.table)[g]);
        if (m == 0) continue;
        U t;
        const U res = residual(a.dense + q * a.s.R * a.s.C, a.s, r, j * kWave + lane, lane, t);
        unsigned long long mine = 0;
        for (U left = m; left; left &= left - 1) {                    // uniform
            const int k = lowest(left);
            const unsigned long long w = __ballot((int)((res >> k) & 1));
            if (lane == k) mine = w;
        }
        const int k = lane & (W - 1);
        if (lane < W && ((m >> k) & 1)) {
            unsigned long long* words = reinterpret_cast<unsigned long long*>(chunk + 2 * a.s.table);
            words[a.count[item] + popc(U(m & ((U(1) << k) - 1)))] = mine;
        }
    }
}

// ---- exclusive scan of count[q][0 .. n), in place, and the chunk sizes ------------------------------------------------------
// exclusive scan of one value per thread over the workgroup; `total` = the sum, in every thread
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long* lds, unsigned long long& total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long x = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += x;
    }
    if (lane == kWave - 1) lds[wave] = inc;
    __syncthreads();
    unsigned long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; w++) {
        if (w < wave) before += lds[w];
        total += lds[w];
    }
    __syncthreads();
    return before + inc - v;
}

// workgroup (q, b): the sum of tile b of plane q
__global__ void __launch_bounds__(kBlock)
k_scan_tiles(const unsigned long long* __restrict__ count, int64_t n, int64_t ntiles, unsigned long long* __restrict__ tile_sum)
{
    __shared__ unsigned long long lds[kWavesPerBlock];
    const int64_t q = blockIdx.x / ntiles, b = blockIdx.x % ntiles;
    const int64_t first = b * kTile + (int64_t)threadIdx.x * kPerThread;
    unsigned long long v = 0, total;
    for (int i = 0; i < kPerThread; i++)
        if (first + i < n) v += count[q * n + first + i];
    (void)block_exclusive(v, lds, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// workgroup q: the exclusive scan of the tile sums of plane q, and what the chunk holds
__global__ void __launch_bounds__(kBlock)
k_scan_top(unsigned long long* __restrict__ tile_sum, int64_t ntiles, uint64_t tables, unsigned long long* __restrict__ sizes)
{
    __shared__ unsigned long long lds[kWavesPerBlock];
    unsigned long long* mine = tile_sum + blockIdx.x * ntiles;
    unsigned long long carry = 0;
    for (int64_t first = 0; first < ntiles; first += kBlock) {
        const int64_t i = first + threadIdx.x;
        const unsigned long long v = i < ntiles ? mine[i] : 0;
        unsigned long long total;
        const unsigned long long before = block_exclusive(v, lds, total);
        if (i < ntiles) mine[i] = carry + before;
        carry += total;
    }
    if (sizes && threadIdx.x == 0) sizes[blockIdx.x] = tables + 8 * carry;
}

__global__ void __launch_bounds__(kBlock)
k_scan_apply(unsigned long long* __restrict__ count, int64_t n, int64_t ntiles, const unsigned long long* __restrict__ tile_sum)
{
    __shared__ unsigned long long lds[kWavesPerBlock];
    const int64_t q = blockIdx.x / ntiles, b = blockIdx.x % ntiles;
    const int64_t first = b * kTile + (int64_t)threadIdx.x * kPerThread;
    unsigned long long c[kPerThread], v = 0, total;
#pragma unroll
    for (int i = 0; i < kPerThread; i++) {
        c[i] = first + i < n ? count[q * n + first + i] : 0;
        v += c[i];
    }
    unsigned long long at = tile_sum[blockIdx.x] + block_exclusive(v, lds, total);
#pragma unroll
    for (int i = 0; i < kPerThread; i++) {
        if (first + i < n) count[q * n + first + i] = at;
        at += c[i];
    }
}

// count[q][n] (popcounts) -> their exclusive scan per plane; sizes[q] (nullable) = tables + 8 x the plane's words
int scan(armon_ctx* ctx, unsigned long long* count, int nplanes, int64_t n, uint64_t tables, unsigned long long* sizes)
{
    const int64_t ntiles = (n + kTile - 1) / kTile;
    unsigned long long* tile_sum = count + (int64_t)nplanes * n;
    const dim3 block(kBlock), tiles((unsigned)(nplanes * ntiles));
    hipLaunchKernelGGL(k_scan_tiles, tiles, block, 0, ctx->stream, count, n, ntiles, tile_sum);
    int rc = check_launch("plane_scan_tiles");
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_scan_top, dim3((unsigned)nplanes), block, 0, ctx->stream, tile_sum, ntiles, tables, sizes);
    rc = check_launch("plane_scan_top");
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_scan_apply, tiles, block, 0, ctx->stream, count, n, ntiles, tile_sum);
    return check_launch("plane_scan_apply");
}

// ---- decode -----------------------------------------------------------------------------------------------------------------
template <typename U>
struct dec_args {
    const unsigned char* chunk;
    uint64_t chunk_bytes;
    unsigned long long* count;   // [n]: exclusive scan of the popcounts of the mask table
    shape s;
    int64_t col0, row0, snx, sny;
    int64_t rb0, gc0, ngc;       // first row block, first group column, group columns of the sub-window
    int64_t items;               // (row blocks) x (group columns) of the sub-window
    U* out;                      // [sny][snx]
    unsigned int* status;
};

template <typename U>
__global__ void __launch_bounds__(kBlock)
k_plane_popcounts(const U* __restrict__ mask, int64_t n, unsigned long long* __restrict__ count)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        count[i] = (unsigned long long)popc(mask[i]);
}

template <typename U>
__global__ void __launch_bounds__(kBlock)
k_plane_decode(dec_args<U> a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const U* base = reinterpret_cast<const U*>(a.chunk);
    const U* mask = reinterpret_cast<const U*>(a.chunk + a.s.table);
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(a.chunk + 2 * a.s.table);
    const int64_t row_end = a.row0 + a.sny;
    for (int64_t item = wave; item < a.items; item += nwaves) {       // wave-uniform
        const int64_t b = a.rb0 + item / a.ngc, j = a.gc0 + item % a.ngc, c = j * kWave + lane;
        const int64_t last = (b + 1) * kRowBlock < row_end ? (b + 1) * kRowBlock : row_end;
        const bool mine = c >= a.col0 && c < a.col0 + a.snx;          // (the sub-window lies inside the plane)
        U above = 0;
        for (int64_t r = b * kRowBlock; r < last; r++) {
            const int64_t g = r * a.s.G + j;
            const U m = uniform(mask[g]);
            U res = 0;
            if (m != 0) {                                             // uniform
                const unsigned long long at = uniform(a.count[g]);
                const int pc = popc(m);
                if (2 * a.s.table + 8 * (at + (unsigned long long)pc) > a.chunk_bytes) {
                    if (lane == 0) *a.status = 1;
                } else {
                    const unsigned long long w = lane < pc ? words[at + lane] : 0;
                    int i = 0;
                    for (U left = m; left; left &= left - 1, i++) {
                        const unsigned long long wi = __shfl(w, i, kWave);
                        res |= U((wi >> lane) & 1) << lowest(left);
                    }
                }
            }
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const U x = __shfl_up(res, d, kWave);
                if (lane >= d) res ^= x;
            }
            const U u = res ^ base[g] ^ above;
            above = u;
            if (mine && r >= a.row0) a.out[(r - a.row0) * a.snx + (c - a.col0)] = u;
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int make_shape(int elem_bytes, int64_t rows, int64_t wnx, shape& s)
{
    ARMON_REQUIRE(rows >= 1 && wnx >= 1, "invalid plane: %lld rows x %lld columns", (long long)rows, (long long)wnx);
    ARMON_REQUIRE(rows < (1ll << 31) && wnx < (1ll << 31), "plane too large: %lld rows x %lld columns", (long long)rows, (long long)wnx);
    s.R = rows; s.C = wnx;
    s.G = (wnx + kWave - 1) / kWave;
    s.n = rows * s.G;
    ARMON_REQUIRE(s.n < (1ll << 36), "plane too large: %lld groups", (long long)s.n);
    s.table = pad8((uint64_t)s.n * elem_bytes);
    return ARMON_OK;
}

uint64_t bound_of(const shape& s, int elem_bytes) { return 2 * s.table + 8ull * (8 * elem_bytes) * (uint64_t)s.n; }

int64_t wave_blocks(armon_ctx* ctx, int64_t items)
{
    const int64_t blocks = (items + kWavesPerBlock - 1) / kWavesPerBlock, most = (int64_t)ctx->n_cu * 8;
    return blocks < most ? blocks : most;
}

// the scan's scratch: the counts of every plane, then a sum per tile
int scan_scratch(armon_ctx* ctx, int nplanes, int64_t n, unsigned long long*& count)
{
    const int rc = ensure_partials(ctx, (size_t)nplanes * (n + (n + kTile - 1) / kTile));      // (doubles and 64-bit words have the same size)
    count = reinterpret_cast<unsigned long long*>(ctx->partials);
    return rc;
}

template <typename T>
int encode_impl(armon_ctx* ctx, const T* dense_dev, int nplanes, int64_t rows, int64_t wnx, void* out_dev, uint64_t plane_capacity,
                uint64_t* sizes_dev)
{
    typedef typename bits<T>::type U;
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(dense_dev && out_dev && sizes_dev, "NULL argument");
    ARMON_REQUIRE(nplanes >= 1 && nplanes <= kMaxPlanes, "nplanes = %d: 1 to %d planes", nplanes, kMaxPlanes);
    enc_args<U> a;
    int rc = make_shape((int)sizeof(U), rows, wnx, a.s);
    if (rc != ARMON_OK) return rc;
    ARMON_REQUIRE(plane_capacity % 8 == 0 && plane_capacity >= bound_of(a.s, (int)sizeof(U)),
                  "plane_capacity = %llu: a multiple of 8 and at least the bound %llu", (unsigned long long)plane_capacity,
                  (unsigned long long)bound_of(a.s, (int)sizeof(U)));
    ARMON_REQUIRE((uintptr_t)out_dev % 8 == 0 && (uintptr_t)dense_dev % sizeof(U) == 0, "misaligned buffer");
    rc = scan_scratch(ctx, nplanes, a.s.n, a.count);
    if (rc != ARMON_OK) return rc;
    a.dense = reinterpret_cast<const U*>(dense_dev);
    a.out = static_cast<unsigned char*>(out_dev);
    a.capacity = plane_capacity;
    a.nplanes = nplanes;
    const dim3 grid((unsigned)wave_blocks(ctx, nplanes * a.s.n)), block(kBlock);
    hipLaunchKernelGGL(k_plane_masks<U>, grid, block, 0, ctx->stream, a);
    rc = check_launch("plane_masks");
    if (rc != ARMON_OK) return rc;
    rc = scan(ctx, a.count, nplanes, a.s.n, 2 * a.s.table, reinterpret_cast<unsigned long long*>(sizes_dev));
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_plane_emit<U>, grid, block, 0, ctx->stream, a);
    return check_launch("plane_emit");
}

template <typename T>
int decode_impl(armon_ctx* ctx, const void* chunk_dev, uint64_t chunk_bytes, int64_t rows, int64_t wnx, int64_t col0, int64_t row0,
                int64_t snx, int64_t sny, T* out_dev, uint32_t* status_dev)
{
    typedef typename bits<T>::type U;
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(chunk_dev && out_dev && status_dev, "NULL argument");
    dec_args<U> a;
    int rc = make_shape((int)sizeof(U), rows, wnx, a.s);
    if (rc != ARMON_OK) return rc;
    ARMON_REQUIRE(col0 >= 0 && row0 >= 0 && snx >= 1 && sny >= 1 && snx <= wnx - col0 && sny <= rows - row0,
                  "the sub-window [%lld, %lld) x [%lld, %lld) leaves the chunk of %lld x %lld", (long long)col0,
                  (long long)(col0 + snx), (long long)row0, (long long)(row0 + sny), (long long)wnx, (long long)rows);
    ARMON_REQUIRE(chunk_bytes >= 2 * a.s.table, "chunk_bytes = %llu: the tables of this shape take %llu",
                  (unsigned long long)chunk_bytes, (unsigned long long)(2 * a.s.table));
    ARMON_REQUIRE((uintptr_t)chunk_dev % 8 == 0 && (uintptr_t)out_dev % sizeof(U) == 0, "misaligned buffer");
    rc = scan_scratch(ctx, 1, a.s.n, a.count);
    if (rc != ARMON_OK) return rc;
    a.chunk = static_cast<const unsigned char*>(chunk_dev);
    a.chunk_bytes = chunk_bytes;
    a.col0 = col0; a.row0 = row0; a.snx = snx; a.sny = sny;
    a.rb0 = row0 / kRowBlock;
    a.gc0 = col0 / kWave;
    a.ngc = (col0 + snx - 1) / kWave - a.gc0 + 1;
    a.items = ((row0 + sny - 1) / kRowBlock - a.rb0 + 1) * a.ngc;
    a.out = reinterpret_cast<U*>(out_dev);
    a.status = status_dev;
    const dim3 block(kBlock);
    const int64_t pblocks = (a.s.n + kBlock - 1) / kBlock, most = (int64_t)ctx->n_cu * 8;
    hipLaunchKernelGGL(k_plane_popcounts<U>, dim3((unsigned)(pblocks < most ? pblocks : most)), block, 0, ctx->stream,
                       reinterpret_cast<const U*>(a.chunk + a.s.table), a.s.n, a.count);
    rc = check_launch("plane_popcounts");
    if (rc != ARMON_OK) return rc;
    rc = scan(ctx, a.count, 1, a.s.n, 2 * a.s.table, nullptr);
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_plane_decode<U>, dim3((unsigned)wave_blocks(ctx, a.items)), block, 0, ctx->stream, a);
    return check_launch("plane_decode");
}

}  // namespace

extern "C" {

uint64_t armon_hip_plane_encode_bound(int elem_bytes, int64_t rows, int64_t wnx)
{
    shape s;
    if ((elem_bytes != 4 && elem_bytes != 8) || make_shape(elem_bytes, rows, wnx, s) != ARMON_OK) return 0;
    return bound_of(s, elem_bytes);
}

int armon_hip_plane_encode(armon_ctx* ctx, const double* dense_dev, int nplanes, int64_t rows, int64_t wnx, void* out_dev,
                           uint64_t plane_capacity, uint64_t* sizes_dev)
{
    return encode_impl<double>(ctx, dense_dev, nplanes, rows, wnx, out_dev, plane_capacity, sizes_dev);
}
int armon_hip_plane_encode_f32(armon_ctx* ctx, const float* dense_dev, int nplanes, int64_t rows, int64_t wnx, void* out_dev,
                               uint64_t plane_capacity, uint64_t* sizes_dev)
{
    return encode_impl<float>(ctx, dense_dev, nplanes, rows, wnx, out_dev, plane_capacity, sizes_dev);
}

int armon_hip_plane_decode(armon_ctx* ctx, const void* chunk_dev, uint64_t chunk_bytes, int64_t rows, int64_t wnx, int64_t col0,
                           int64_t row0, int64_t snx, int64_t sny, double* out_dev, uint32_t* status_dev)
{
    return decode_impl<double>(ctx, chunk_dev, chunk_bytes, rows, wnx, col0, row0, snx, sny, out_dev, status_dev);
}
int armon_hip_plane_decode_f32(armon_ctx* ctx, const void* chunk_dev, uint64_t chunk_bytes, int64_t rows, int64_t wnx, int64_t col0,
                               int64_t row0, int64_t snx, int64_t sny, float* out_dev, uint32_t* status_dev)
{
    return decode_impl<float>(ctx, chunk_dev, chunk_bytes, rows, wnx, col0, row0, snx, sny, out_dev, status_dev);
}

}  // extern "C"
