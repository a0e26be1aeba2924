// derive.hip — derived flow fields for in-situ images: one pass over the real cells of a block turns (rho, u, v, E) into up to
// eight selected quantities per cell and reduces each over the fx x fy coarse cells of armon_hip_coarsen (same cell -> coarse
// cell map, same clamping of a factor larger than the grid). Only the coarse planes [nq][cny][cnx] are written.
//
// No reference counterpart (the reference writes whole fields, ref src/io.jl:2-27).
//
// PER CELL, all arithmetic in the data type T, one IEEE operation per operation written (the library is built with
// -ffp-contract=off; `/` and sqrt are the correctly rounded ones):
//     e          = E - 0.5 (u u + v v)
//     p, c       = phys::perfect_gas / phys::bizarrium of the cell itself (no p vector is read): p = (gamma - 1) rho e,
//                  c = sqrt((gamma p) / rho) for a perfect gas
//     speed      = sqrt(u u + v v),   mach = speed / c
//     d_x f      = (f_R - f_L) / (T(w) dx)    f_R = f[i+1] if that cell exists, else f[i]; f_L likewise; w = how many of the
//                  two exist; w = 0: the derivative is 0 and nothing is divided. d_y likewise with dy.
//                  A neighbour EXISTS if it is a real cell of the block or lies in the first ghost layer of a side whose
//                  bit of `neighbours` is set: central differences inside and across tile edges, one-sided ones at the edge
//                  of the global domain.
//     grad_rho   = sqrt(gx gx + gy gy),   vorticity = d_x v - d_y u,   divergence = d_x u + d_y v
// Only the four edge-adjacent ghost strips of flagged sides are ever read: no corner, no deeper layer, no ghost of an
// unflagged side.
//
// REDUCTION. MEAN = the sum in THE SUMMATION ORDER of csrc/coarsen.hip, restated here, divided by the number of cells covered:
//   1. per column of the coarse cell, the rows are added one after the other, top down, in chunks of kRowChunk rows counted
//      from the coarse cell's first row; the chunk sums of a column are then added in chunk order (one chunk when fy <= 64);
//   2. the column sums c_0 .. c_{fx-1} (c_i = 0 for a column the grid does not have) are combined by a balanced binary tree
//      over the column index padded to the next power of two P; when P > 256, column sums 256 apart are first added in
//      ascending order and the tree runs over those 256 values.
// MAX and MIN run through the same walk with the neutral element -inf / +inf; of two zeros the maximum is +0 and the minimum
// -0, so that they too are functions of the values covered only. A NaN among the covered values gives the canonical quiet NaN
// in all three modes. No atomics.
//
// Two launch forms, as in coarsen.hip. fx a power of two <= 64 and fy <= 64 — ONE kernel, no scratch. Any other factor — the
// same kernel stores the column results of each row chunk to the context's scratch ([nq][cny][nchunk][nx] elements) and a
// second kernel folds them per coarse cell.
//
// Kernel shape. A wave takes 64 lanes x (16 B of columns) x the rows of one (coarse row, row chunk); each lane marches down
// its rows with a rolling window of three rows of rho, u, v in registers (each row of a chunk is loaded once, plus the two
// rows around the chunk: 66 rows read per 64), takes the columns x-1 and x+V from the adjacent lanes with wave shifts (only
// the two lanes at a span's ends load an extra element) and E for the row it evaluates. The lanes, the alignment rule and the
// grid cap (8 workgroups per CU) are those of the window walk (window.hpp) over the whole real domain, with plain loads; the
// item is a (coarse row, row chunk, span). No LDS in the row kernel. It is built
// for up to 2 and up to 8 planes and per EOS form (none needed, perfect gas, Bizarrium): 158 to 192 VGPRs in fp64, 2 to 3
// waves per SIMD — that, not memory, bounds the pass (DESIGN.md §4.9 has the measurements).
#include "physics.hpp"
#include "window.hpp"

#include <cmath>

using namespace armon;

namespace {

constexpr int kRowChunk = 64;
constexpr int kMaxQ = 8;

using win::kWave;
using win::kWavesPerBlock;
using win::wide;

template <typename T>
struct derive_args {
    const T *rho, *u, *v, *E;
    T* out;                         // [nq][cny][cnx]
    T* scratch;                     // two-kernel form: [nq][cny][nchunk][nx] column results of each row chunk
    win::window w;                  // the whole real domain: nx = w.wnx, ny = w.wny
    int64_t fx, fy, cnx, cny;
    int64_t nchunk;                 // row chunks per coarse row
    int tree;                       // single-kernel form: width of the column tree (= fx)
    int nq, quantity[kMaxQ], reduce[kMaxQ];
    int eos, mask;                  // mask: bit Q is set when quantity Q is selected
    int left, right, bottom, top;   // 1: the first ghost layer of that side holds the neighbour tile's cells
    T gamma, dx, dy, dx2, dy2;      // dx2 = T(2) dx
};

__device__ __forceinline__ double qnan(double) { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ float qnan(float) { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ double inf_(double) { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ float inf_(float) { return __uint_as_float(0x7f800000u); }
__device__ __forceinline__ bool neg_(double x) { return __double_as_longlong(x) < 0; }
__device__ __forceinline__ bool neg_(float x) { return (int)__float_as_uint(x) < 0; }
__device__ __forceinline__ double root(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float root(float x) { return __builtin_sqrtf(x); }

template <typename T>
__device__ __forceinline__ T neutral(int mode)
{
    return mode == ARMON_REDUCE_MEAN ? T(0.) : (mode == ARMON_REDUCE_MAX ? -inf_(T(0.)) : inf_(T(0.)));
}

// commutative in all three modes: a sum, or an extremum in which a NaN wins and +0 lies above -0
template <typename T>
__device__ __forceinline__ T combine(int mode, T a, T b)
{
    if (mode == ARMON_REDUCE_MEAN) return a + b;
    if (a != a || b != b) return qnan(T(0.));
    if (mode == ARMON_REDUCE_MAX) return (b > a || (b == a && neg_(a))) ? b : a;
    return (b < a || (b == a && neg_(b))) ? b : a;
}

template <typename T>
__device__ __forceinline__ void store_cell(const derive_args<T>& a, int64_t I, int64_t J, int64_t n, const T s[kMaxQ])
{
    const int64_t plane = a.cnx * a.cny, at = J * a.cnx + I;
#pragma unroll
    for (int q = 0; q < kMaxQ; q++) {
        if (q < a.nq) {
            T r = a.reduce[q] == ARMON_REDUCE_MEAN ? s[q] / T(n) : s[q];
            if (r != r) r = qnan(T(0.));
            a.out[q * plane + at] = r;
        }
    }
}

// one row of rho, u, v as a lane holds it: its V columns, and the column before / after the span (first / last lane only)
template <typename T>
struct row3 {
    T f[3][wide<T>::n];
    T l[3], r[3];
};

// Row r (-1 .. ny) of rho, u, v. A REAL row also takes the ghost column nx when the right side is flagged and the column
// before the span (the ghost column -1 only when the left side is flagged); a ghost row takes its real columns only, so no
// corner is ever read. Columns that may not be read are 0.
template <typename T, bool WIDE>
__device__ __forceinline__ void load_row(const derive_args<T>& a, int64_t r, int64_t x, int lane, row3<T>& w)
{
    constexpr int V = wide<T>::n;
    typedef typename wide<T>::type VT;
    const bool real = r >= 0 && r < a.w.wny;
    const int64_t at = a.w.first + r * a.w.pitch + x;
    const int64_t hi = real ? a.w.wnx + a.right : a.w.wnx;               // columns below `hi` may be read
    const bool whole = x + V <= a.w.wnx;
    const T* const src[3] = {a.rho, a.u, a.v};
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (WIDE && whole) {
            const VT t = *reinterpret_cast<const VT*>(src[q] + at);
#pragma unroll
            for (int c = 0; c < V; c++) w.f[q][c] = t[c];
        } else {
#pragma unroll
            for (int c = 0; c < V; c++) w.f[q][c] = x + c < hi ? src[q][at + c] : T(0.);
        }
        w.l[q] = T(0.);
        w.r[q] = T(0.);
        if (real && lane == 0 && x < a.w.wnx && (x > 0 || a.left)) w.l[q] = src[q][at - 1];
        if (real && lane == kWave - 1 && x + V < hi) w.r[q] = src[q][at + V];
    }
}

template <typename T, bool WIDE>
__device__ __forceinline__ void load_E(const derive_args<T>& a, int64_t r, int64_t x, T e[wide<T>::n])
{
    constexpr int V = wide<T>::n;
    typedef typename wide<T>::type VT;
    const int64_t at = a.w.first + r * a.w.pitch + x;
    if (WIDE && x + V <= a.w.wnx) {
        const VT t = *reinterpret_cast<const VT*>(a.E + at);
#pragma unroll
        for (int c = 0; c < V; c++) e[c] = t[c];
    } else {
#pragma unroll
        for (int c = 0; c < V; c++) e[c] = x + c < a.w.wnx ? a.E[at + c] : T(0.);
    }
}

template <typename T>
__device__ __forceinline__ T deriv(T fl, T fc, T fr, bool has_l, bool has_r, T d1, T d2)
{
    const int w = (int)has_l + (int)has_r;
    if (w == 0) return T(0.);
    const T hi = has_r ? fr : fc, lo = has_l ? fl : fc;
    return (hi - lo) / (w == 2 ? d2 : d1);
}

constexpr int kStencil = (1 << ARMON_DERIVE_GRAD_RHO) | (1 << ARMON_DERIVE_VORTICITY) | (1 << ARMON_DERIVE_DIVERGENCE);
constexpr int kNeedsEos = (1 << ARMON_DERIVE_P) | (1 << ARMON_DERIVE_MACH);
constexpr int kNeedsE = kNeedsEos | (1 << ARMON_DERIVE_EINT);

// Column results over the rows of one (coarse row, row chunk, span) per wave. FINISH: the single-kernel form.
// EOS: 0 = neither p nor the Mach number is selected, 1 = perfect gas, 2 = Bizarrium — a build of its own each, so that
// the registers of the Bizarrium evaluation do not set the occupancy of a schlieren frame.
template <typename T, bool WIDE, bool FINISH, int NQ, int EOS>
__global__ void __launch_bounds__(kBlock)
k_derive_rows(derive_args<T> a)
{
    constexpr int V = wide<T>::n;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t units = a.cny * a.nchunk * a.w.nspan;
    const bool stencil = (a.mask & kStencil) != 0, with_E = (a.mask & kNeedsE) != 0;
    for (int64_t unit = wave; unit < units; unit += nwaves) {      // wave-uniform, and so is everything that shuffles below
        const int64_t s = unit % a.w.nspan, jk = unit / a.w.nspan, k = jk % a.nchunk, J = jk / a.nchunk;
        const auto [x, left] = win::lane_column<V>(a.w, s, lane);
        const int64_t r_end = (J + 1) * a.fy < a.w.wny ? (J + 1) * a.fy : a.w.wny;
        const int64_t r_lo = J * a.fy + k * kRowChunk;
        const int64_t r_hi = r_lo + kRowChunk < r_end ? r_lo + kRowChunk : r_end;
        T acc[NQ][V];
#pragma unroll
        for (int q = 0; q < NQ; q++)
#pragma unroll
            for (int c = 0; c < V; c++) acc[q][c] = neutral<T>(q < a.nq ? a.reduce[q] : 0);
        row3<T> below, cur, above;                                  // rows r - 1, r, r + 1
#pragma unroll
        for (int q = 0; q < 3; q++) {
#pragma unroll
            for (int c = 0; c < V; c++) below.f[q][c] = above.f[q][c] = T(0.);
            below.l[q] = below.r[q] = above.l[q] = above.r[q] = T(0.);
        }
        // (the last coarse row may be partial: a chunk past its end has no row at all, r_lo >= r_hi, and loads nothing)
        bool has_below = stencil && (r_lo > 0 || a.bottom);
        if (r_lo < r_hi) {                                          // wave-uniform
            if (has_below) load_row<T, WIDE>(a, r_lo - 1, x, lane, below);
            load_row<T, WIDE>(a, r_lo, x, lane, cur);
        } else {
#pragma unroll
            for (int q = 0; q < 3; q++) {
#pragma unroll
                for (int c = 0; c < V; c++) cur.f[q][c] = T(0.);
                cur.l[q] = cur.r[q] = T(0.);
            }
        }
        for (int64_t r = r_lo; r < r_hi; r++) {
            const bool has_above = stencil && (r + 1 < a.w.wny || a.top);
            if (has_above) load_row<T, WIDE>(a, r + 1, x, lane, above);
            else if (r + 1 < r_hi) load_row<T, WIDE>(a, r + 1, x, lane, above);        // (pointwise quantities only)
            T e_tot[V];
#pragma unroll
            for (int c = 0; c < V; c++) e_tot[c] = T(0.);
            if (with_E) load_E<T, WIDE>(a, r, x, e_tot);
            // the columns x - 1 and x + V of this row: from the adjacent lanes, or what the span's end lanes loaded
            T lv[3], rv[3];
#pragma unroll
            for (int q = 0; q < 3; q++) {
                lv[q] = __shfl_up(cur.f[q][V - 1], 1, kWave);
                rv[q] = __shfl_down(cur.f[q][0], 1, kWave);
                if (lane == 0) lv[q] = cur.l[q];
                if (lane == kWave - 1) rv[q] = cur.r[q];
            }
#pragma unroll
            for (int c = 0; c < V; c++) {
                const int64_t col = x + c;
                const bool in = col < a.w.wnx;
                const T rho = cur.f[0][c], u = cur.f[1][c], v = cur.f[2][c], E = e_tot[c];
                T d[ARMON_DERIVE_COUNT];
#pragma unroll
                for (int i = 0; i < ARMON_DERIVE_COUNT; i++) d[i] = T(0.);
                d[ARMON_DERIVE_RHO] = rho;
                if (a.mask & (1 << ARMON_DERIVE_EINT)) d[ARMON_DERIVE_EINT] = E - T(0.5) * (u * u + v * v);
                const T speed = root(u * u + v * v);
                d[ARMON_DERIVE_SPEED] = speed;
                if (EOS != 0) {
                    T p, cs, g;
                    if (EOS == 1) phys::perfect_gas<T>(a.gamma, rho, E, u, v, p, cs);
                    else phys::bizarrium<false, T>(rho, E, u, v, p, cs, g);
                    d[ARMON_DERIVE_P] = p;
                    d[ARMON_DERIVE_MACH] = speed / cs;
                }
                if (stencil) {
                    const bool has_l = col > 0 || a.left, has_r = col + 1 < a.w.wnx || a.right;
                    T fl[3], fr[3];
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        fl[q] = c > 0 ? cur.f[q][c > 0 ? c - 1 : 0] : lv[q];
                        fr[q] = c < V - 1 ? cur.f[q][c < V - 1 ? c + 1 : c] : rv[q];
                    }
                    if (a.mask & (1 << ARMON_DERIVE_GRAD_RHO)) {
                        const T gx = deriv(fl[0], rho, fr[0], has_l, has_r, a.dx, a.dx2);
                        const T gy = deriv(below.f[0][c], rho, above.f[0][c], has_below, has_above, a.dy, a.dy2);
                        d[ARMON_DERIVE_GRAD_RHO] = root(gx * gx + gy * gy);
                    }
                    if (a.mask & (1 << ARMON_DERIVE_VORTICITY))
                        d[ARMON_DERIVE_VORTICITY] = deriv(fl[2], v, fr[2], has_l, has_r, a.dx, a.dx2) -
                                                    deriv(below.f[1][c], u, above.f[1][c], has_below, has_above, a.dy, a.dy2);
                    if (a.mask & (1 << ARMON_DERIVE_DIVERGENCE))
                        d[ARMON_DERIVE_DIVERGENCE] = deriv(fl[1], u, fr[1], has_l, has_r, a.dx, a.dx2) +
                                                     deriv(below.f[2][c], v, above.f[2][c], has_below, has_above, a.dy, a.dy2);
                }
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    if (q < a.nq) {
                        const T val = d[a.quantity[q]];             // (a wave-uniform index)
                        if (in) acc[q][c] = combine(a.reduce[q], acc[q][c], val);
                    }
                }
            }
            below = cur;
            cur = above;
            has_below = stencil;                                   // row r is real
        }
        if (FINISH) {
            // the balanced tree over the columns of a coarse cell: inside the lane, then across lanes
#pragma unroll
            for (int w = 1; w < V; w *= 2) {
                if (w < a.tree) {
#pragma unroll
                    for (int c = 0; c < V; c += 2 * w)
#pragma unroll
                        for (int q = 0; q < NQ; q++)
                            if (q < a.nq) acc[q][c] = combine(a.reduce[q], acc[q][c], acc[q][c + w]);
                }
            }
            const int lanes = a.tree > V ? a.tree / V : 1;         // lanes per coarse cell
            for (int off = 1; off < lanes; off *= 2) {
#pragma unroll
                for (int q = 0; q < NQ; q++)
                    if (q < a.nq) acc[q][0] = combine(a.reduce[q], acc[q][0], __shfl_xor(acc[q][0], off, kWave));
            }
            if ((lane & (lanes - 1)) == 0) {
#pragma unroll
                for (int c = 0; c < V; c++) {
                    if (c % a.tree == 0 && x + c < a.w.wnx) {
                        const int64_t I = (x + c) / a.fx;
                        const int64_t nc = (I + 1) * a.fx < a.w.wnx ? a.fx : a.w.wnx - I * a.fx;
                        T res[kMaxQ];
#pragma unroll
                        for (int q = 0; q < kMaxQ; q++) res[q] = q < NQ ? acc[q < NQ ? q : 0][c] : T(0.);
                        store_cell(a, I, J, nc * (r_hi - r_lo), res);
                    }
                }
            }
        } else if (left > 0) {
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                if (q < a.nq) {
                    T* __restrict__ dst = a.scratch + ((q * a.cny + J) * a.nchunk + k) * a.w.wnx + x;
#pragma unroll
                    for (int c = 0; c < V; c++)
                        if (x + c < a.w.wnx) dst[c] = acc[q][c];
                }
            }
        }
    }
}

// Second kernel of the two-kernel form: a team of `team` threads (a power of two <= 256) per coarse cell folds the chunk
// results of each column in chunk order, columns `team` apart in ascending order, then runs the tree over the team.
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_derive_cols(derive_args<T> a, int team)
{
    __shared__ T lds[kMaxQ][kWavesPerBlock];
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
        T acc[kMaxQ];
#pragma unroll
        for (int q = 0; q < kMaxQ; q++) acc[q] = neutral<T>(q < a.nq ? a.reduce[q] : 0);
        for (int64_t i = t; i < nc; i += team) {
#pragma unroll
            for (int q = 0; q < kMaxQ; q++) {
                if (q < a.nq) {
                    T col = neutral<T>(a.reduce[q]);
                    for (int64_t k = 0; k < kn; k++)
                        col = combine(a.reduce[q], col, scratch[((q * a.cny + J) * a.nchunk + k) * a.w.wnx + x0 + i]);
                    acc[q] = combine(a.reduce[q], acc[q], col);
                }
            }
        }
        const int in_wave = team < kWave ? team : kWave;
        for (int off = 1; off < in_wave; off *= 2) {
#pragma unroll
            for (int q = 0; q < kMaxQ; q++)
                if (q < a.nq) acc[q] = combine(a.reduce[q], acc[q], __shfl_xor(acc[q], off, kWave));
        }
        if (team > kWave) {                                                 // uniform
            if ((tid & (kWave - 1)) == 0) {
#pragma unroll
                for (int q = 0; q < kMaxQ; q++) lds[q][tid / kWave] = acc[q];
            }
            __syncthreads();
            if (t == 0) {
                const int w0 = tid / kWave;
#pragma unroll
                for (int q = 0; q < kMaxQ; q++) {
                    if (q < a.nq) {
                        const int m = a.reduce[q];
                        acc[q] = team == 2 * kWave ? combine(m, lds[q][w0], lds[q][w0 + 1])
                                                   : combine(m, combine(m, lds[q][0], lds[q][1]), combine(m, lds[q][2], lds[q][3]));
                    }
                }
            }
            __syncthreads();
        }
        if (valid && t == 0) store_cell(a, I, J, nc * nr, acc);
    }
}

inline bool is_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

template <typename T>
int derive_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
                const T* rho, const T* u, const T* v, const T* E, const armon_derive_spec* spec, T* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(fx >= 1 && fy >= 1, "coarsening factors must be >= 1, got (%lld, %lld)", (long long)fx, (long long)fy);
    derive_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, 0, 0, nx, ny, a.w);
    if (rc != ARMON_OK) return rc;
    ARMON_REQUIRE(rho && u && v && E && spec && out_dev, "NULL argument");
    const armon_derive_spec& s = *spec;
    ARMON_REQUIRE(s.nq >= 1 && s.nq <= kMaxQ, "derive: nq = %d: 1 to %d quantities", s.nq, kMaxQ);
    ARMON_REQUIRE(s.eos == ARMON_EOS_PERFECT_GAS || s.eos == ARMON_EOS_BIZARRIUM, "unknown eos %d", s.eos);
    ARMON_REQUIRE((s.neighbours & ~15) == 0, "derive: neighbours = %d has bits other than left, right, bottom, top", s.neighbours);
    ARMON_REQUIRE(s.neighbours == 0 || nghost >= 1, "derive: neighbours = %d needs a ghost layer, nghost = %d", s.neighbours, nghost);
    ARMON_REQUIRE(std::isfinite(s.dx) && std::isfinite(s.dy) && s.dx > 0 && s.dy > 0 && std::isfinite((T)s.dx) && std::isfinite((T)s.dy) &&
                  (T)s.dx > 0 && (T)s.dy > 0, "derive: dx = %g, dy = %g must be finite and > 0", s.dx, s.dy);
    a.mask = 0;
    for (int q = 0; q < kMaxQ; q++) {
        a.quantity[q] = a.reduce[q] = 0;
        if (q >= s.nq) continue;
        ARMON_REQUIRE(s.quantity[q] >= 0 && s.quantity[q] < ARMON_DERIVE_COUNT, "derive: unknown quantity %d", s.quantity[q]);
        ARMON_REQUIRE(s.reduce[q] == ARMON_REDUCE_MEAN || s.reduce[q] == ARMON_REDUCE_MAX || s.reduce[q] == ARMON_REDUCE_MIN,
                      "derive: unknown reduction %d", s.reduce[q]);
        a.quantity[q] = s.quantity[q];
        a.reduce[q] = s.reduce[q];
        a.mask |= 1 << s.quantity[q];
    }
    const bool single = is_pow2(fx) && fx <= kWave && fy <= kRowChunk;
    a.rho = rho; a.u = u; a.v = v; a.E = E;
    a.out = out_dev;
    a.scratch = nullptr;
    // a factor larger than the grid makes one coarse cell along that axis: index arithmetic with the clamped value
    a.fx = single || fx < nx ? fx : nx;
    a.fy = fy < ny ? fy : ny;
    a.cnx = (nx + a.fx - 1) / a.fx;
    a.cny = (ny + a.fy - 1) / a.fy;
    a.nchunk = (a.fy + kRowChunk - 1) / kRowChunk;
    a.tree = single ? (int)fx : 0;
    a.nq = s.nq;
    a.eos = s.eos;
    a.left = s.neighbours & 1; a.right = (s.neighbours >> 1) & 1; a.bottom = (s.neighbours >> 2) & 1; a.top = (s.neighbours >> 3) & 1;
    a.gamma = (T)s.gamma; a.dx = (T)s.dx; a.dy = (T)s.dy;
    a.dx2 = T(2.) * a.dx; a.dy2 = T(2.) * a.dy;
    const uintptr_t mis = (uintptr_t)rho | (uintptr_t)u | (uintptr_t)v | (uintptr_t)E;
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n);
    const int64_t units = a.cny * a.nchunk * a.w.nspan, max_blocks = (int64_t)ctx->n_cu * 8;
    int64_t blocks = (units + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > max_blocks) blocks = max_blocks;
    if (!single) {
        // one value per real column, row chunk and quantity: nq * nx * ceil(ny / min(fy, 64)) elements (include/armon_hip.h)
        const size_t bytes = (size_t)a.nq * a.cny * a.nchunk * a.w.wnx * sizeof(T);
        rc = ensure_partials(ctx, (bytes + sizeof(double) - 1) / sizeof(double));   // grows (and waits) on first need only
        if (rc != ARMON_OK) return rc;
        a.scratch = reinterpret_cast<T*>(ctx->partials);
    }
    const dim3 grid((unsigned)blocks), block(kBlock);
    // the row kernel is built for 2 and 8 planes and per EOS: a frame of one or two quantities does not pay for eight accumulators
    const int eos_form = (a.mask & kNeedsEos) == 0 ? 0 : (a.eos == ARMON_EOS_PERFECT_GAS ? 1 : 2);
#define ARMON_DERIVE_ROWS_2(W, F, NQ)                                                                                        \
    do {                                                                                                                     \
        if (eos_form == 0) hipLaunchKernelGGL((k_derive_rows<T, W, F, NQ, 0>), grid, block, 0, ctx->stream, a);              \
        else if (eos_form == 1) hipLaunchKernelGGL((k_derive_rows<T, W, F, NQ, 1>), grid, block, 0, ctx->stream, a);         \
        else hipLaunchKernelGGL((k_derive_rows<T, W, F, NQ, 2>), grid, block, 0, ctx->stream, a);                            \
    } while (0)
#define ARMON_DERIVE_ROWS(W, F)                                                                                              \
    do {                                                                                                                     \
        if (a.nq <= 2) ARMON_DERIVE_ROWS_2(W, F, 2);                                                                         \
        else ARMON_DERIVE_ROWS_2(W, F, kMaxQ);                                                                               \
    } while (0)
    if (single) {
        if (wide_ok) ARMON_DERIVE_ROWS(true, true);
        else ARMON_DERIVE_ROWS(false, true);
        return check_launch("derive");
    }
    if (wide_ok) ARMON_DERIVE_ROWS(true, false);
    else ARMON_DERIVE_ROWS(false, false);
#undef ARMON_DERIVE_ROWS
#undef ARMON_DERIVE_ROWS_2
    rc = check_launch("derive_rows");
    if (rc != ARMON_OK) return rc;
    int team = 1;
    while (team < kBlock && team < fx) team *= 2;
    const int64_t ncell = a.cnx * a.cny, teams = kBlock / team;
    int64_t groups = (ncell + teams - 1) / teams;
    if (groups > max_blocks) groups = max_blocks;
    hipLaunchKernelGGL(k_derive_cols<T>, dim3((unsigned)groups), block, 0, ctx->stream, a, team);
    return check_launch("derive_cols");
}

}  // namespace

extern "C" {

int armon_hip_derive(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
                     const double* rho, const double* u, const double* v, const double* E, const armon_derive_spec* spec,
                     double* out_dev)
{
    return derive_impl<double>(ctx, row_length, nghost, nx, ny, fx, fy, rho, u, v, E, spec, out_dev);
}

int armon_hip_derive_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
                         const float* rho, const float* u, const float* v, const float* E, const armon_derive_spec* spec,
                         float* out_dev)
{
    return derive_impl<float>(ctx, row_length, nghost, nx, ny, fx, fy, rho, u, v, E, spec, out_dev);
}

}  // extern "C"
