// coarsen.hip — in-situ reduced output: conservative block-averaging of the state and a strided gather.
//
// No reference counterpart (the reference writes whole fields, ref src/io.jl:2-27). Both kernels exist so that an output
// never moves a full field to the host: a coarse cell (I, J) of factors (fx, fy) covers the real cells
// i in [I fx, min((I+1) fx, nx)), j in [J fy, min((J+1) fy, ny)) — n of them — and gets
//     rho = S(rho) / n,   u = S(rho u) / S(rho),   v = S(rho v) / S(rho),   E = S(rho E) / S(rho),   p = S(p) / n.
//
// THE SUMMATION ORDER is a function of (fx, fy) and of the cells covered only — not of where the cells sit in memory, of
// the alignment path, of the grid size or of the launch shape:
//   1. per column of the coarse cell, the rows are added one after the other, top down, in chunks of kRowChunk rows counted
//      from the coarse cell's first row; the chunk sums of a column are then added in chunk order (one chunk when fy <= 64);
//   2. the column sums c_0 .. c_{fx-1} (c_i = 0 for a column the grid does not have) are combined by a balanced binary tree
//      over the column index padded to the next power of two P: (c_0 + c_1) + (c_2 + c_3) ...; when P > 256, column sums
//      256 apart are first added in ascending order (t, t + 256, ...) and the tree runs over those 256 values.
// Floating-point addition is commutative, so the xor butterfly that evaluates the tree gives every lane those very bits.
// No atomics. Products and sums are never contracted (the library is built with -ffp-contract=off).
//
// Two launch forms. fx a power of two <= 64 and fy <= 64 — ONE kernel: a wave takes 64 lanes x (16 B of columns) x the fy
// rows of one coarse row, each lane adds its rows in registers, the columns are combined in the lane and then across lanes
// (__shfl_xor), the first lane of each coarse cell divides and stores. Any other factor — the same
// kernel stores the column sums of each row chunk to the context's scratch and a second kernel folds them per coarse cell
// (a team of min(P, 256) threads per cell). The lanes, the alignment rule and the grid cap (8 workgroups per CU) are those of
// the window walk (window.hpp) over the whole real domain, with plain loads; the item is a (coarse row, row chunk, span).
#include "window.hpp"

using namespace armon;

namespace {

constexpr int kRowChunk = 64;
constexpr int kMaxGather = 8;

using win::kWave;
using win::kWavesPerBlock;
using win::wide;

template <typename T>
struct coarsen_args {
    const T *rho, *u, *v, *E, *p;   // p may be NULL
    T* out;                         // [5][cny][cnx]
    T* scratch;                     // two-kernel form: [5][cny][nchunk][nx] column sums of each row chunk
    win::window w;                  // the whole real domain: nx = w.wnx, ny = w.wny
    int64_t fx, fy, cnx, cny;
    int64_t nchunk;                 // row chunks per coarse row
    int tree;                       // single-kernel form: width of the column tree (= fx)
};

template <typename T>
__device__ __forceinline__ void store_cell(const coarsen_args<T>& a, int64_t I, int64_t J, int64_t n, const T s[5])
{
    const int64_t plane = a.cnx * a.cny, at = J * a.cnx + I;
    a.out[at] = s[0] / T(n);
    a.out[plane + at] = s[1] / s[0];
    a.out[2 * plane + at] = s[2] / s[0];
    a.out[3 * plane + at] = s[3] / s[0];
    if (a.p) a.out[4 * plane + at] = s[4] / T(n);
}

// Column sums over the rows of one (coarse row, row chunk, span) per wave. WIDE: every row of the real domain starts on a
// 16-B boundary in all the vectors — one 16-B load per vector, row and lane; otherwise the same lanes take the same
// columns with element-wide loads. FINISH: the single-kernel form.
template <typename T, bool WIDE, bool FINISH>
__global__ void __launch_bounds__(kBlock)
k_coarsen_rows(coarsen_args<T> a)
{
    constexpr int V = wide<T>::n;
    typedef typename wide<T>::type VT;
    const T* __restrict__ rho = a.rho;
    const T* __restrict__ u = a.u;
    const T* __restrict__ v = a.v;
    const T* __restrict__ E = a.E;
    const T* __restrict__ p = a.p;
    const bool has_p = p != nullptr;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t units = a.cny * a.nchunk * a.w.nspan;
    for (int64_t unit = wave; unit < units; unit += nwaves) {      // wave-uniform
        const int64_t s = unit % a.w.nspan, jk = unit / a.w.nspan, k = jk % a.nchunk, J = jk / a.nchunk;
        const auto [x, left] = win::lane_column<V>(a.w, s, lane);
        const int64_t r_end = (J + 1) * a.fy < a.w.wny ? (J + 1) * a.fy : a.w.wny;
        const int64_t r_lo = J * a.fy + k * kRowChunk;
        const int64_t r_hi = r_lo + kRowChunk < r_end ? r_lo + kRowChunk : r_end;
        T acc[5][V];
#pragma unroll
        for (int q = 0; q < 5; q++)
#pragma unroll
            for (int c = 0; c < V; c++) acc[q][c] = T(0.);
        const bool whole = left >= V;
        if (left > 0) {
#pragma unroll 4
            for (int64_t r = r_lo; r < r_hi; r++) {
                const int64_t at = a.w.first + r * a.w.pitch + x;
                T f[5][V];
                if (WIDE && whole) {
                    const VT w0 = *reinterpret_cast<const VT*>(rho + at), w1 = *reinterpret_cast<const VT*>(u + at);
                    const VT w2 = *reinterpret_cast<const VT*>(v + at), w3 = *reinterpret_cast<const VT*>(E + at);
                    VT w4 = VT(T(0.));
                    if (has_p) w4 = *reinterpret_cast<const VT*>(p + at);
#pragma unroll
                    for (int c = 0; c < V; c++) { f[0][c] = w0[c]; f[1][c] = w1[c]; f[2][c] = w2[c]; f[3][c] = w3[c]; f[4][c] = w4[c]; }
                } else {
#pragma unroll
                    for (int c = 0; c < V; c++) {
                        const bool in = x + c < a.w.wnx;             // columns past the real domain are ghosts: never read
                        f[0][c] = in ? rho[at + c] : T(0.);
                        f[1][c] = in ? u[at + c] : T(0.);
                        f[2][c] = in ? v[at + c] : T(0.);
                        f[3][c] = in ? E[at + c] : T(0.);
                        f[4][c] = in && has_p ? p[at + c] : T(0.);
                    }
                }
#pragma unroll
                for (int c = 0; c < V; c++) {
                    acc[0][c] += f[0][c];
                    acc[1][c] += f[0][c] * f[1][c];
                    acc[2][c] += f[0][c] * f[2][c];
                    acc[3][c] += f[0][c] * f[3][c];
                    acc[4][c] += f[4][c];
                }
            }
        }
        if (FINISH) {
            // the balanced tree over the columns of a coarse cell: inside the lane, then across lanes
#pragma unroll
            for (int w = 1; w < V; w *= 2) {
                if (w < a.tree) {
#pragma unroll
                    for (int c = 0; c < V; c += 2 * w)
#pragma unroll
                        for (int q = 0; q < 5; q++) acc[q][c] += acc[q][c + w];
                }
            }
            const int lanes = a.tree > V ? a.tree / V : 1;         // lanes per coarse cell
            for (int off = 1; off < lanes; off *= 2) {
#pragma unroll
                for (int q = 0; q < 5; q++) acc[q][0] += __shfl_xor(acc[q][0], off, kWave);
            }
            if ((lane & (lanes - 1)) == 0) {
#pragma unroll
                for (int c = 0; c < V; c++) {
                    if (c % a.tree == 0 && x + c < a.w.wnx) {
                        const int64_t I = (x + c) / a.fx;
                        const int64_t nc = (I + 1) * a.fx < a.w.wnx ? a.fx : a.w.wnx - I * a.fx;
                        const T sums[5] = {acc[0][c], acc[1][c], acc[2][c], acc[3][c], acc[4][c]};
                        store_cell(a, I, J, nc * (r_hi - r_lo), sums);
                    }
                }
            }
        } else if (left > 0) {
#pragma unroll
            for (int q = 0; q < 5; q++) {
                if (q == 4 && !has_p) break;
                T* __restrict__ dst = a.scratch + ((q * a.cny + J) * a.nchunk + k) * a.w.wnx + x;
#pragma unroll
                for (int c = 0; c < V; c++)
                    if (x + c < a.w.wnx) dst[c] = acc[q][c];
            }
        }
    }
}

// Second kernel of the two-kernel form: a team of `team` threads (a power of two <= 256) per coarse cell adds the chunk
// sums of each column in chunk order, columns `team` apart in ascending order, then runs the tree over the team.
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_coarsen_cols(coarsen_args<T> a, int team)
{
    __shared__ T lds[5][kWavesPerBlock];
    const bool has_p = a.p != nullptr;
    const int tid = threadIdx.x, teams = kBlock / team, my_team = tid / team, t = tid % team;
    const int64_t ncell = a.cnx * a.cny, ngroups = (ncell + teams - 1) / teams;
    const T* __restrict__ scratch = a.scratch;
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {      // workgroup-uniform
        const int64_t cell = grp * teams + my_team;
        const bool valid = cell < ncell;
        const int64_t I = valid ? cell % a.cnx : 0, J = valid ? cell / a.cnx : 0;
        const int64_t x0 = I * a.fx, y0 = J * a.fy;
        const int64_t nc = valid ? (x0 + a.fx < a.w.wnx ? a.fx : a.w.wnx - x0) : 0;
        const int64_t nr = y0 + a.fy < a.w.wny ? a.fy : a.w.wny - y0;
        const int64_t kn = (nr + kRowChunk - 1) / kRowChunk;
        T acc[5] = {T(0.), T(0.), T(0.), T(0.), T(0.)};
        for (int64_t i = t; i < nc; i += team) {
            T col[5] = {T(0.), T(0.), T(0.), T(0.), T(0.)};
            for (int64_t k = 0; k < kn; k++) {
#pragma unroll
                for (int q = 0; q < 5; q++)
                    if (q < 4 || has_p) col[q] += scratch[((q * a.cny + J) * a.nchunk + k) * a.w.wnx + x0 + i];
            }
#pragma unroll
            for (int q = 0; q < 5; q++) acc[q] += col[q];
        }
        const int in_wave = team < kWave ? team : kWave;
        for (int off = 1; off < in_wave; off *= 2) {
#pragma unroll
            for (int q = 0; q < 5; q++) acc[q] += __shfl_xor(acc[q], off, kWave);
        }
        if (team > kWave) {                                                 // uniform
            if ((tid & (kWave - 1)) == 0) {
#pragma unroll
                for (int q = 0; q < 5; q++) lds[q][tid / kWave] = acc[q];
            }
            __syncthreads();
            if (t == 0) {
                const int w0 = tid / kWave;
#pragma unroll
                for (int q = 0; q < 5; q++)
                    acc[q] = team == 2 * kWave ? lds[q][w0] + lds[q][w0 + 1] : (lds[q][0] + lds[q][1]) + (lds[q][2] + lds[q][3]);
            }
            __syncthreads();
        }
        if (valid && t == 0) store_cell(a, I, J, nc * nr, acc);
    }
}

template <typename T>
struct gather_args { const T* vars[kMaxGather]; };

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_gather_strided(gather_args<T> g, int nvars, int64_t start, int64_t stride, int64_t count, T* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        for (int q = 0; q < nvars; q++) out[q * count + i] = g.vars[q][start + i * stride];
    }
}

inline bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

template <typename T>
int coarsen_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
                 const T* rho, const T* u, const T* v, const T* E, const T* p, T* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(fx >= 1 && fy >= 1, "coarsening factors must be >= 1, got (%lld, %lld)", (long long)fx, (long long)fy);
    coarsen_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, 0, 0, nx, ny, a.w);
    if (rc != ARMON_OK) return rc;
    ARMON_REQUIRE(rho && u && v && E && out_dev, "NULL array");
    const bool single = is_pow2(fx) && fx <= kWave && fy <= kRowChunk;
    a.rho = rho; a.u = u; a.v = v; a.E = E; a.p = p;
    a.out = out_dev;
    a.scratch = nullptr;
    // a factor larger than the grid makes one coarse cell along that axis: index arithmetic with the clamped value
    a.fx = single || fx < nx ? fx : nx;
    a.fy = fy < ny ? fy : ny;
    a.cnx = (nx + a.fx - 1) / a.fx;
    a.cny = (ny + a.fy - 1) / a.fy;
    a.nchunk = (a.fy + kRowChunk - 1) / kRowChunk;
    a.tree = single ? (int)fx : 0;
    const uintptr_t mis = (uintptr_t)rho | (uintptr_t)u | (uintptr_t)v | (uintptr_t)E | (uintptr_t)p;
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n);
    const int64_t units = a.cny * a.nchunk * a.w.nspan, max_blocks = (int64_t)ctx->n_cu * 8;
    int64_t blocks = (units + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > max_blocks) blocks = max_blocks;
    if (!single) {
        // one value per real column, row chunk and plane: nx * ceil(ny / min(fy, 64)) * 4 (5 with p) elements — as much as
        // the fields themselves when fy = 1. It stays with the context (include/armon_hip.h says so).
        const size_t bytes = (size_t)(p ? 5 : 4) * a.cny * a.nchunk * a.w.wnx * sizeof(T);
        rc = ensure_partials(ctx, (bytes + sizeof(double) - 1) / sizeof(double));   // grows (and waits) on first need only
        if (rc != ARMON_OK) return rc;
        a.scratch = reinterpret_cast<T*>(ctx->partials);
    }
    const dim3 grid((unsigned)blocks), block(kBlock);
    if (single) {
        if (wide_ok) hipLaunchKernelGGL((k_coarsen_rows<T, true, true>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_coarsen_rows<T, false, true>), grid, block, 0, ctx->stream, a);
        return check_launch("coarsen");
    }
    if (wide_ok) hipLaunchKernelGGL((k_coarsen_rows<T, true, false>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_coarsen_rows<T, false, false>), grid, block, 0, ctx->stream, a);
    rc = check_launch("coarsen_rows");
    if (rc != ARMON_OK) return rc;
    int team = 1;
    while (team < kBlock && team < fx) team *= 2;
    const int64_t ncell = a.cnx * a.cny, teams = kBlock / team;
    int64_t groups = (ncell + teams - 1) / teams;
    if (groups > max_blocks) groups = max_blocks;
    hipLaunchKernelGGL(k_coarsen_cols<T>, dim3((unsigned)groups), block, 0, ctx->stream, a, team);
    return check_launch("coarsen_cols");
}

template <typename T>
int gather_strided_impl(armon_ctx* ctx, int64_t n_cells, int nvars, const T* const* vars, int64_t start, int64_t stride,
                        int64_t count, T* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nvars >= 1 && nvars <= kMaxGather, "nvars = %d: 1 to %d vectors", nvars, kMaxGather);
    ARMON_REQUIRE(vars && out_dev, "NULL argument");
    ARMON_REQUIRE(count >= 0 && start >= 0 && stride >= 1 && n_cells >= 0, "invalid slice: start = %lld, stride = %lld, count = %lld",
                  (long long)start, (long long)stride, (long long)count);
    if (count == 0) return ARMON_OK;
    ARMON_REQUIRE(start < n_cells && (count - 1) <= (n_cells - 1 - start) / stride,
                  "the slice leaves the block: start = %lld, stride = %lld, count = %lld, %lld cells",
                  (long long)start, (long long)stride, (long long)count, (long long)n_cells);
    gather_args<T> g;
    for (int q = 0; q < kMaxGather; q++) {
        g.vars[q] = q < nvars ? vars[q] : nullptr;
        ARMON_REQUIRE(q >= nvars || vars[q], "NULL array");
    }
    int64_t blocks = (count + kBlock - 1) / kBlock;
    if (blocks > (int64_t)ctx->n_cu * 8) blocks = (int64_t)ctx->n_cu * 8;
    hipLaunchKernelGGL(k_gather_strided<T>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, g, nvars, start, stride, count, out_dev);
    return check_launch("gather_strided");
}

}  // namespace

#define ARMON_EXPORT(name, impl, PARAMS, ARGS)                                            \
    int armon_hip_##name(PARAMS(double)) { return impl<double> ARGS; }                    \
    int armon_hip_##name##_f32(PARAMS(float)) { return impl<float> ARGS; }

extern "C" {

#define P_CO(T) armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy, \
                const T* rho, const T* u, const T* v, const T* E, const T* p, T* out_dev
ARMON_EXPORT(coarsen, coarsen_impl, P_CO, (ctx, row_length, nghost, nx, ny, fx, fy, rho, u, v, E, p, out_dev))

#define P_GS(T) armon_ctx* ctx, int64_t n_cells, int nvars, const T* const* vars, int64_t start, int64_t stride, int64_t count, T* out_dev
ARMON_EXPORT(gather_strided, gather_strided_impl, P_GS, (ctx, n_cells, nvars, vars, start, stride, count, out_dev))

}  // extern "C"
