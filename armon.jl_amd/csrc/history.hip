// history.hip — the run over time, on the device: armon_hip_history_sample reduces a window of real cells to one 320-byte
// record (armon_history_record, include/armon_hip.h: six exact sums, eight extrema with their cells) and gathers up to 64
// point gauges, into a slot of a ring that lives on the device and is read back in batches (armon_hip_history_read). Nothing
// is moved: rho, u, v, E are read once (32 B per fp64 cell), only the slot is written.
//
// No reference counterpart: the reference prints mass and energy per cycle behind a fence (ref src/solver.jl:356-371).
//
// PER CELL (the full rule is in the header; armon.jl_amd/history.py restates it in Python and the tests hold this file against
// that): q2 = u u + v v, e = E - 0.5 q2, (p, c) = the EOS in the data type; the terms rho, rho u, rho v, rho E, (0.5 rho) q2, p
// enter exact sums (exact_sum.hpp), rho, p, e a pair minimum and maximum, q2 and q2 / (c c) a pair maximum. All of it fp64 but
// the EOS, no contraction (-ffp-contract=off for the whole library), IEEE division.
//
// MERGE: integer addition, pair minimum and pair maximum only — associative and commutative, so the record is a function of
// the state and the scale: not of the launch shape, the alignment path, the ghost width or the decomposition.
//
// STREAM-ORDERED: a sample is two launches on the context's stream and returns; the host never waits for it. The scratch
// between the two belongs to the handle (sized at creation), not to the context: ensure_partials may move the context's
// while a run is in flight, and the dt partials of the fused sweep live there.
//
// Launch: the window walk of window.hpp, the four loads of an item issued before its arithmetic, kPerCu workgroups per CU. A
// lane keeps its 36 words in registers; wave shuffle -> LDS over the four waves -> one partial of 36 words per workgroup ->
// k_history_fold, one workgroup, merges them and WRITES the slot, then its first lanes gather the gauges. No atomics.
#include "exact_sum.hpp"

#include <cmath>

using namespace armon;

namespace {

constexpr int kTerms = 6, kExt = 8;
constexpr int kSums = 2 + 3 * kTerms;       // n, n_bad, 6 x 3 limbs
constexpr int kWords = kSums + 2 * kExt;    // words of a partial: 36
constexpr int kRecWords = 40;               // sizeof(armon_history_record) / 8
constexpr int kGaugeWords = 5;
constexpr int kPerCu = 3;                   // workgroups per CU: what 150 to 160 VGPRs allow (launch bounds below)

using exact::u64;
using exact::u128;
using exact::quantise;
using red::op_pair_min;
using red::order_key;
using win::bits_of;
using win::finite;
using win::kNone;
using win::kWave;
using win::kWavesPerBlock;
using win::load_cells;
using win::pick;
using win::wide;

static_assert(sizeof(armon_history_record) == kRecWords * 8, "armon_history_record is 40 words");
static_assert(sizeof(armon_history_spec) == 48, "armon_history_spec is 48 bytes");

__device__ __forceinline__ bool is_min_ext(int k) { return k == ARMON_HISTORY_RHO_MIN || k == ARMON_HISTORY_P_MIN || k == ARMON_HISTORY_E_MIN; }

template <typename T>
struct hist_args {
    const T *rho, *u, *v, *E;
    win::window w;
    int64_t gx0, gy0;               // global position of the window's first cell
    armon_history_spec s;
    u64* partials;                  // [gridDim.x][kWords]
};

template <typename T>
__device__ __forceinline__ void eos_of(const armon_history_spec& s, T rho, T u, T v, T E, T& p, T& c)
{
    if (s.eos == ARMON_EOS_PERFECT_GAS) phys::perfect_gas<T>((T)s.gamma, rho, E, u, v, p, c);
    else { T g; phys::bizarrium<false, T>(rho, E, u, v, p, c, g); }
}

struct hist_acc {
    u64 n, n_bad;
    long long sum[kTerms][3];
    red::upair ext[kExt];
};

template <typename T>
__device__ __forceinline__ void add_cell(const armon_history_spec& s, T rho_, T u_, T v_, T E_, u64 g, hist_acc& acc)
{
    const double rho = (double)rho_, u = (double)u_, v = (double)v_, E = (double)E_;
    const double q2 = u * u + v * v;
    const double e = E - 0.5 * q2;
    T p_, c_;
    eos_of<T>(s, rho_, u_, v_, E_, p_, c_);
    const double p = (double)p_, c = (double)c_;
    const double t[kTerms] = {rho, rho * u, rho * v, rho * E, (0.5 * rho) * q2, p};
    const double m = q2 == 0. ? 0. : q2 / (c * c);
    bool ok = finite(rho) && finite(u) && finite(v) && finite(E) && finite(e) && finite(c);
    u128 a[kTerms];
#pragma unroll
    for (int k = 0; k < kTerms; k++) ok = quantise(t[k], s.scale_exp[k], a[k]) && ok;        // (false for a term that is not finite)
    // no branch from here on: a bad cell adds zeros and neutral pairs
    acc.n += ok ? 1 : 0;
    acc.n_bad += ok ? 0 : 1;
#pragma unroll
    for (int k = 0; k < kTerms; k++) exact::add_limbs(acc.sum[k], ok ? a[k] : (u128)0, bits_of(t[k]) >> 63);
    const double x[kExt] = {rho, rho, p, p, e, e, q2, m};
#pragma unroll
    for (int k = 0; k < kExt; k++) {
        if (is_min_ext(k)) acc.ext[k] = op_pair_min::f(acc.ext[k], red::upair{ok ? order_key(x[k]) : kNone, ok ? g : kNone});
        else acc.ext[k] = red::op_pair_max::f(acc.ext[k], red::upair{ok ? order_key(x[k]) : 0ull, ok ? g : kNone});
    }
}

template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock, kPerCu)
k_history(hist_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 lds[kWavesPerBlock][kWords];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const T* __restrict__ rho = a.rho + a.w.first;
    const T* __restrict__ u = a.u + a.w.first;
    const T* __restrict__ v = a.v + a.w.first;
    const T* __restrict__ E = a.E + a.w.first;
    hist_acc acc;
    acc.n = acc.n_bad = 0;
#pragma unroll
    for (int k = 0; k < kTerms; k++) acc.sum[k][0] = acc.sum[k][1] = acc.sum[k][2] = 0;
#pragma unroll
    for (int k = 0; k < kExt; k++) acc.ext[k] = is_min_ext(k) ? red::upair{kNone, kNone} : red::upair{0, kNone};
    win::walk<V>(a.w, [&](int64_t r, int64_t x, int64_t left) {
        if (left <= 0) return;
        T fr[V], fu[V], fv[V], fE[V];                               // the four loads are issued before the first arithmetic
        const int64_t at = r * a.w.pitch + x;
        load_cells<T, WIDE>(rho + at, left >= V, left, fr);
        load_cells<T, WIDE>(u + at, left >= V, left, fu);
        load_cells<T, WIDE>(v + at, left >= V, left, fv);
        load_cells<T, WIDE>(E + at, left >= V, left, fE);
        const u64 g = (u64)(a.gy0 + r) * (u64)a.s.global_nx + (u64)(a.gx0 + x);
#pragma nounroll                                                    // one copy of the cell's arithmetic next to the 72 accumulator registers
        for (int c = 0; c < V; c++) {
            if (c >= left) break;
            add_cell<T>(a.s, pick<V>(fr, c), pick<V>(fu, c), pick<V>(fv, c), pick<V>(fE, c), g + (u64)c, acc);
        }
    });
    // lane -> wave -> LDS -> one partial per workgroup
    {
        u64* row = lds[w];
        const u64 n = red::wave_reduce<red::op_sum>(acc.n), n_bad = red::wave_reduce<red::op_sum>(acc.n_bad);
        if (lane == 0) { row[0] = n; row[1] = n_bad; }
#pragma unroll
        for (int j = 0; j < 3 * kTerms; j++) {
            const u64 sum = red::wave_reduce<red::op_sum>((u64)acc.sum[j / 3][j % 3]);
            if (lane == 0) row[2 + j] = sum;
        }
#pragma unroll
        for (int k = 0; k < kExt; k++) {
            const red::upair m = is_min_ext(k) ? red::wave_reduce<op_pair_min>(acc.ext[k]) : red::wave_reduce<red::op_pair_max>(acc.ext[k]);
            if (lane == 0) { row[kSums + 2 * k] = m.v; row[kSums + 2 * k + 1] = m.at; }
        }
    }
    __syncthreads();
    u64* part = a.partials + (int64_t)blockIdx.x * kWords;
    if (tid < kSums) {
        u64 sum = 0;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; i++) sum += lds[i][tid];
        part[tid] = sum;
    } else if (tid < kSums + kExt) {
        const int k = tid - kSums, at = kSums + 2 * k;
        red::upair m = is_min_ext(k) ? red::upair{kNone, kNone} : red::upair{0, kNone};
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; i++) {
            const red::upair o{lds[i][at], lds[i][at + 1]};
            m = is_min_ext(k) ? op_pair_min::f(m, o) : red::op_pair_max::f(m, o);
        }
        part[at] = m.v;
        part[at + 1] = m.at;
    }
}

template <typename T>
struct fold_args {
    const T *rho, *u, *v, *E;
    int64_t pitch, first, wnx;
    armon_history_spec s;
    const u64* partials;
    int n_partials;
    u64* slot;                      // [kRecWords + kGaugeWords x max_gauges]
    const int64_t* cells;           // [n_gauges]: row * wnx + col in the window, or -1
    int n_gauges, max_gauges;
};

// one workgroup: slot = merge(the partials), then the gauges
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_history_fold(fold_args<T> a)
{
    __shared__ u64 lds[kWavesPerBlock];
    __shared__ red::upair lds_pair[kWavesPerBlock];
    const int tid = (int)threadIdx.x;
    u64 sum[kSums];
    red::upair ext[kExt];
#pragma unroll
    for (int j = 0; j < kSums; j++) sum[j] = 0;
#pragma unroll
    for (int k = 0; k < kExt; k++) ext[k] = is_min_ext(k) ? red::upair{kNone, kNone} : red::upair{0, kNone};
    for (int i = tid; i < a.n_partials; i += kBlock) {
        const u64* p = a.partials + (int64_t)i * kWords;
#pragma unroll
        for (int j = 0; j < kSums; j++) sum[j] += p[j];
#pragma unroll
        for (int k = 0; k < kExt; k++) {
            const red::upair o{p[kSums + 2 * k], p[kSums + 2 * k + 1]};
            ext[k] = is_min_ext(k) ? op_pair_min::f(ext[k], o) : red::op_pair_max::f(ext[k], o);
        }
    }
#pragma unroll
    for (int j = 0; j < kSums; j++) sum[j] = red::block_reduce<red::op_sum, kWavesPerBlock>(sum[j], lds, tid);
#pragma unroll
    for (int k = 0; k < kExt; k++)
        ext[k] = is_min_ext(k) ? red::block_reduce<op_pair_min, kWavesPerBlock>(ext[k], lds_pair, tid)
                               : red::block_reduce<red::op_pair_max, kWavesPerBlock>(ext[k], lds_pair, tid);
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < kSums; j++) a.slot[j] = sum[j];
#pragma unroll
        for (int k = 0; k < kExt; k++) { a.slot[kSums + 2 * k] = ext[k].v; a.slot[kSums + 2 * k + 1] = ext[k].at; }
#pragma unroll
        for (int j = kWords; j < kRecWords; j++) a.slot[j] = 0;
    }
    if (tid < a.max_gauges) {
        double* out = reinterpret_cast<double*>(a.slot + kRecWords) + (int64_t)tid * kGaugeWords;
        const int64_t cell = tid < a.n_gauges ? a.cells[tid] : -1;
        double val[kGaugeWords] = {0., 0., 0., 0., 0.};
        if (cell >= 0) {                                            // (< wnx wny: checked by the host before the launch)
            const int64_t at = a.first + (cell / a.wnx) * a.pitch + cell % a.wnx;
            const T rho = a.rho[at], u = a.u[at], v = a.v[at], E = a.E[at];
            T p, c;
            eos_of<T>(a.s, rho, u, v, E, p, c);
            val[0] = (double)rho; val[1] = (double)u; val[2] = (double)v; val[3] = (double)E; val[4] = (double)p;
        }
#pragma unroll
        for (int j = 0; j < kGaugeWords; j++) out[j] = val[j];
    }
}

}  // namespace

struct armon_history {
    armon_ctx* ctx = nullptr;
    int capacity = 0, max_gauges = 0, n_gauges = 0;
    int64_t slot_words = 0;
    int max_blocks = 0;             // workgroups the partials hold
    u64* ring = nullptr;            // [capacity][slot_words]
    u64* partials = nullptr;        // [max_blocks][kWords]
    int64_t* cells_dev = nullptr;   // [max_gauges]
    u64* landing = nullptr;         // pinned, [capacity][slot_words]
    int64_t cells[ARMON_HISTORY_MAX_GAUGES];
};

namespace {

void release(armon_history* h)
{
    if (h->ring) (void)hipFree(h->ring);
    if (h->partials) (void)hipFree(h->partials);
    if (h->cells_dev) (void)hipFree(h->cells_dev);
    if (h->landing) (void)hipHostFree(h->landing);
    delete h;
}

template <typename T>
int sample_impl(armon_ctx* ctx, armon_history* h, int slot, const armon_history_spec* spec, int64_t row_length, int nghost, int64_t nx,
                int64_t ny, const T* rho, const T* u, const T* v, const T* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny,
                int64_t global_col0, int64_t global_row0)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(h && rho && u && v && E && spec, "NULL argument");
    ARMON_REQUIRE(h->ctx == ctx, "history: the handle belongs to another context");
    ARMON_REQUIRE(slot >= 0 && slot < h->capacity, "history: slot %d outside the ring of %d", slot, h->capacity);
    hist_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
    if (rc == ARMON_OK) rc = win::check_global_cell(global_col0, global_row0);
    if (rc != ARMON_OK) return rc;
    const armon_history_spec& s = *spec;
    ARMON_REQUIRE(s.eos == ARMON_EOS_PERFECT_GAS || s.eos == ARMON_EOS_BIZARRIUM, "unknown eos %d", s.eos);
    ARMON_REQUIRE(s.eos != ARMON_EOS_PERFECT_GAS || (std::isfinite(s.gamma) && s.gamma > 1), "history: gamma = %g", s.gamma);
    ARMON_REQUIRE(s.global_nx >= global_col0 + wnx && s.global_nx < (1ll << 40), "history: global_nx = %lld", (long long)s.global_nx);
    for (int k = 0; k < kTerms; k++)
        ARMON_REQUIRE(s.scale_exp[k] >= -4096 && s.scale_exp[k] <= 4096, "history: scale_exp[%d] = %d leaves [-4096, 4096]", k, s.scale_exp[k]);
    for (int i = 0; i < h->n_gauges; i++)
        ARMON_REQUIRE(h->cells[i] < wnx * wny, "history: gauge %d sits at cell %lld of a window of %lld", i, (long long)h->cells[i],
                      (long long)(wnx * wny));
    a.rho = rho; a.u = u; a.v = v; a.E = E;
    a.gx0 = global_col0; a.gy0 = global_row0;
    a.s = s;
    a.partials = h->partials;
    const uintptr_t mis = (uintptr_t)rho | (uintptr_t)u | (uintptr_t)v | (uintptr_t)E;
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n);
    const int64_t blocks = win::walk_blocks(a.w, h->max_blocks);
    const dim3 grid((unsigned)blocks), block(kBlock);
    if (wide_ok) hipLaunchKernelGGL((k_history<T, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_history<T, false>), grid, block, 0, ctx->stream, a);
    rc = check_launch("history");
    if (rc != ARMON_OK) return rc;
    fold_args<T> f;
    f.rho = rho; f.u = u; f.v = v; f.E = E;
    f.pitch = a.w.pitch; f.first = a.w.first; f.wnx = wnx;
    f.s = s;
    f.partials = h->partials;
    f.n_partials = (int)blocks;
    f.slot = h->ring + (int64_t)slot * h->slot_words;
    f.cells = h->cells_dev;
    f.n_gauges = h->n_gauges; f.max_gauges = h->max_gauges;
    hipLaunchKernelGGL(k_history_fold<T>, dim3(1), block, 0, ctx->stream, f);
    return check_launch("history_fold");
}

}  // namespace

extern "C" {

int armon_hip_history_create(armon_ctx* ctx, int capacity, int max_gauges, armon_history** out)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(out, "history_create: out is NULL");
    *out = nullptr;
    ARMON_REQUIRE(capacity >= 1 && capacity <= 65536, "history_create: capacity = %d leaves [1, 65536]", capacity);
    ARMON_REQUIRE(max_gauges >= 0 && max_gauges <= ARMON_HISTORY_MAX_GAUGES, "history_create: max_gauges = %d leaves [0, %d]", max_gauges,
                  ARMON_HISTORY_MAX_GAUGES);
    ARMON_REQUIRE(!ctx->capturing, "history_create inside a stream capture");
    ARMON_HIP_TRY(hipSetDevice(ctx->device));
    armon_history* h = new armon_history();
    h->ctx = ctx;
    h->capacity = capacity;
    h->max_gauges = max_gauges;
    h->slot_words = kRecWords + (int64_t)kGaugeWords * max_gauges;
    h->max_blocks = (ctx->n_cu > 0 ? ctx->n_cu : 1) * kPerCu;
    const size_t ring_bytes = (size_t)capacity * h->slot_words * 8;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->ring), ring_bytes);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->partials), (size_t)h->max_blocks * kWords * 8);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->cells_dev), sizeof(int64_t) * ARMON_HISTORY_MAX_GAUGES);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h->landing), ring_bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(h->ring, 0, ring_bytes, ctx->stream);
    if (e != hipSuccess) {
        release(h);
        return fail_hip(e, "history_create");
    }
    *out = h;
    return ARMON_OK;
}

int armon_hip_history_destroy(armon_ctx* ctx, armon_history* h)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    if (!h) return ARMON_OK;
    ARMON_REQUIRE(h->ctx == ctx, "history: the handle belongs to another context");
    ARMON_HIP_TRY(hipStreamSynchronize(ctx->stream));       // a sample or a read may still be queued
    release(h);
    return ARMON_OK;
}

int armon_hip_history_set_gauges(armon_ctx* ctx, armon_history* h, const int64_t* cells, int n)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(h && (cells || n == 0), "NULL argument");
    ARMON_REQUIRE(h->ctx == ctx, "history: the handle belongs to another context");
    ARMON_REQUIRE(n >= 0 && n <= h->max_gauges, "history: %d gauges, the handle holds %d", n, h->max_gauges);
    for (int i = 0; i < n; i++) ARMON_REQUIRE(cells[i] >= -1, "history: gauge %d has the cell %lld", i, (long long)cells[i]);
    ARMON_HIP_TRY(hipStreamSynchronize(ctx->stream));       // queued samples read the table
    for (int i = 0; i < n; i++) h->cells[i] = cells[i];
    h->n_gauges = n;
    if (n > 0) {
        ARMON_HIP_TRY(hipMemcpyAsync(h->cells_dev, h->cells, sizeof(int64_t) * n, hipMemcpyHostToDevice, ctx->stream));
        ARMON_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return ARMON_OK;
}

int armon_hip_history_sample(armon_ctx* ctx, armon_history* h, int slot, const armon_history_spec* spec, int64_t row_length, int nghost,
                             int64_t nx, int64_t ny, const double* rho, const double* u, const double* v, const double* E, int64_t col0,
                             int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0)
{
    return sample_impl<double>(ctx, h, slot, spec, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0);
}

int armon_hip_history_sample_f32(armon_ctx* ctx, armon_history* h, int slot, const armon_history_spec* spec, int64_t row_length, int nghost,
                                 int64_t nx, int64_t ny, const float* rho, const float* u, const float* v, const float* E, int64_t col0,
                                 int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0)
{
    return sample_impl<float>(ctx, h, slot, spec, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0);
}

int armon_hip_history_read(armon_ctx* ctx, armon_history* h, int first_slot, int count, armon_history_record* records_host,
                           double* gauges_host)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(h, "history_read: the handle is NULL");
    ARMON_REQUIRE(h->ctx == ctx, "history: the handle belongs to another context");
    ARMON_REQUIRE(first_slot >= 0 && count >= 0 && count <= h->capacity - first_slot, "history_read: slots [%d, %d + %d) leave the ring of %d",
                  first_slot, first_slot, count, h->capacity);
    if (count == 0) return ARMON_OK;
    const u64* src = h->ring + (int64_t)first_slot * h->slot_words;
    ARMON_HIP_TRY(hipMemcpyAsync(h->landing, src, (size_t)count * h->slot_words * 8, hipMemcpyDeviceToHost, ctx->stream));
    ARMON_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t gauge_bytes = (size_t)kGaugeWords * h->max_gauges * 8;
    for (int i = 0; i < count; i++) {
        const u64* slot = h->landing + (int64_t)i * h->slot_words;
        if (records_host) memcpy(records_host + i, slot, sizeof(armon_history_record));
        if (gauges_host && gauge_bytes) memcpy(reinterpret_cast<char*>(gauges_host) + i * gauge_bytes, slot + kRecWords, gauge_bytes);
    }
    return ARMON_OK;
}

}  // extern "C"
