// init_regions.hip — user-defined initial states: a background and a list of regions (half-plane, box, disc, ellipse), each
// with its own state, turned into rho, u, v, E from the GLOBAL position of every cell only. No reference
// counterpart: the reference's users add a TestCase subtype in Julia.
//
// The table of regions (at most 32 x 72 bytes) travels as a kernel argument: no device allocation, no upload, no
// synchronisation. The loop over it has a wave-uniform counter, so every region is read with scalar loads.
#include <cmath>

#include "common.hpp"
#include "range_walk.hpp"

using namespace armon;

namespace {

constexpr int kMaxRegions = 32;
constexpr int kMaxSamples = 8;

template <typename T> struct region_t { int32_t kind, reserved; T a[4]; T rho, u, v, E; };
static_assert(sizeof(region_t<double>) == sizeof(armon_region) && sizeof(region_t<float>) == sizeof(armon_region_f32),
              "the kernel's region is the header's");

template <typename T> struct region_table {
    int32_t n, samples;
    T frac[kMaxSamples];         // (2 i + 1) / (2 samples)
    T bg[4];                     // rho, u, v, E
    region_t<T> r[kMaxRegions];
};

// One IEEE operation per operation written (the library is built with -ffp-contract=off); inclusive comparisons.
template <typename T>
__device__ __forceinline__ bool region_holds(const region_t<T>& g, T xs, T ys)
{
    switch (g.kind) {
    case ARMON_REGION_HALF_PLANE: return g.a[0] * xs + g.a[1] * ys <= g.a[2];
    case ARMON_REGION_BOX:        return g.a[0] <= xs && xs <= g.a[1] && g.a[2] <= ys && ys <= g.a[3];
    case ARMON_REGION_DISC:       return (xs - g.a[0]) * (xs - g.a[0]) + (ys - g.a[1]) * (ys - g.a[1]) <= g.a[2];
    case ARMON_REGION_ELLIPSE:    return (xs - g.a[0]) * (xs - g.a[0]) * g.a[2] + (ys - g.a[1]) * (ys - g.a[1]) * g.a[3] <= T(1);
    default:                      return false;
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
k_init_regions(armon_range r, int64_t row_length, int nghost, int64_t gpos_x, int64_t gpos_y, T ox, T oy, T dXx, T dXy,
               region_table<T> tab, T* __restrict__ rho, T* __restrict__ u, T* __restrict__ v, T* __restrict__ E)
{
    ARMON_FOR_RANGE(r, i) {
        int64_t Iy = i / row_length;
        int64_t Ix = i - Iy * row_length - nghost + 1;
        Iy = Iy - nghost + 1;
        const int64_t gx = Ix + gpos_x - 1, gy = Iy + gpos_y - 1;
        const T x = (T)gx * dXx + ox;           // init_test's own cell corner
        const T y = (T)gy * dXy + oy;
        T m = 0, mu = 0, mv = 0, mE = 0;
        T s_rho = 0, s_u = 0, s_v = 0, s_E = 0;
        int first = -2;
        bool mixed = false;
        for (int sy = 0; sy < tab.samples; sy++) {
            const T ys = y + dXy * tab.frac[sy];
            for (int sx = 0; sx < tab.samples; sx++) {
                const T xs = x + dXx * tab.frac[sx];
                // the last region of the list that holds the point: walked from the back, the first hit is kept
                int hit = -1;
                s_rho = tab.bg[0]; s_u = tab.bg[1]; s_v = tab.bg[2]; s_E = tab.bg[3];
                for (int k = tab.n - 1; k >= 0; k--) {
                    if (hit < 0 && region_holds(tab.r[k], xs, ys)) {
                        hit = k;
                        s_rho = tab.r[k].rho; s_u = tab.r[k].u; s_v = tab.r[k].v; s_E = tab.r[k].E;
                    }
                }
                if (first == -2) first = hit;
                mixed = mixed || hit != first;
                m += s_rho;
                mu += s_rho * s_u;
                mv += s_rho * s_v;
                mE += s_rho * s_E;
            }
        }
        if (mixed) {                            // the conservative mix of mass, momentum and total energy
            rho[i] = m / T(tab.samples * tab.samples);
            u[i] = mu / m;
            v[i] = mv / m;
            E[i] = mE / m;
        } else {                                // every sample in one region (or none): its state, verbatim
            rho[i] = s_rho;
            u[i] = s_u;
            v[i] = s_v;
            E[i] = s_E;
        }
    }
}

// SCALAR: the plane of a passive scalar in the slot of rho (armon_hip_init_scalar_regions) — any finite value, either sign
template <typename T, typename R, bool SCALAR = false>
int init_regions_impl(armon_ctx* ctx, armon_range r, int64_t row_length, int nghost, const int64_t global_pos[2],
                      const T origin[2], const T dX[2], int samples, const T background[4], int nregions, const R* regions,
                      T* rho, T* u, T* v, T* E)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(range_ok(r), "invalid range (col %lld:%lld:%lld row %lld+%lld)", (long long)r.col_start,
                  (long long)r.col_step, (long long)r.col_len, (long long)r.row_start, (long long)r.row_len);
    ARMON_REQUIRE(global_pos && origin && dX && background, "NULL argument");
    ARMON_REQUIRE(rho && u && v && E, "NULL array");
    ARMON_REQUIRE(row_length > 0 && nghost >= 0, "invalid row_length %lld / nghost %d", (long long)row_length, nghost);
    ARMON_REQUIRE(nregions >= 0 && nregions <= kMaxRegions, "%d regions: 0 to %d are supported", nregions, kMaxRegions);
    ARMON_REQUIRE(nregions == 0 || regions != nullptr, "NULL region list");
    ARMON_REQUIRE(samples == 1 || samples == 2 || samples == 4 || samples == 8, "samples must be 1, 2, 4 or 8, got %d", samples);
    for (int d = 0; d < 2; d++)
        ARMON_REQUIRE(std::isfinite(origin[d]) && std::isfinite(dX[d]) && dX[d] > 0, "origin / dX must be finite, dX > 0");
    static_assert(sizeof(R) == sizeof(region_t<T>), "region layout");
    region_table<T> tab = {};
    tab.n = nregions;
    tab.samples = samples;
    for (int s = 0; s < samples; s++) tab.frac[s] = T((2 * s + 1) / (2.0 * samples));
    for (int k = 0; k < 4; k++) {
        ARMON_REQUIRE(std::isfinite(background[k]), "the background state holds a NaN or an infinity");
        tab.bg[k] = background[k];
    }
    ARMON_REQUIRE(SCALAR || background[0] > 0, "the background state has rho <= 0");
    for (int k = 0; k < nregions; k++) {
        region_t<T> g;
        memcpy(&g, &regions[k], sizeof(g));
        ARMON_REQUIRE(g.kind >= ARMON_REGION_HALF_PLANE && g.kind <= ARMON_REGION_ELLIPSE, "region %d: unknown kind %d", k, g.kind);
        for (int j = 0; j < 4; j++) {
            ARMON_REQUIRE(!std::isnan(g.a[j]), "region %d: parameter %d is a NaN", k, j);
            ARMON_REQUIRE(g.kind == ARMON_REGION_BOX || !std::isinf(g.a[j]),
                          "region %d: parameter %d is infinite (only the bounds of a box may be)", k, j);
        }
        ARMON_REQUIRE(std::isfinite(g.rho) && std::isfinite(g.u) && std::isfinite(g.v) && std::isfinite(g.E),
                      "region %d: its state holds a NaN or an infinity", k);
        ARMON_REQUIRE(SCALAR || g.rho > 0, "region %d: rho <= 0", k);
        g.reserved = 0;
        tab.r[k] = g;
    }
    if (range_empty(r)) return ARMON_OK;
    dim3 grid, block;
    range_grid(r, 1, grid, block);
    hipLaunchKernelGGL(k_init_regions<T>, grid, block, 0, ctx->stream, r, row_length, nghost, global_pos[0], global_pos[1],
                       origin[0], origin[1], dX[0], dX[1], tab, rho, u, v, E);
    return check_launch("init_regions");
}

}  // namespace

extern "C" {

int armon_hip_init_regions(armon_ctx* ctx, armon_range r, int64_t row_length, int nghost, const int64_t global_pos[2],
                           const double origin[2], const double dX[2], int samples, const double background[4], int nregions,
                           const armon_region* regions, double* rho, double* u, double* v, double* E)
{
    return init_regions_impl<double>(ctx, r, row_length, nghost, global_pos, origin, dX, samples, background, nregions, regions,
                                     rho, u, v, E);
}

int armon_hip_init_regions_f32(armon_ctx* ctx, armon_range r, int64_t row_length, int nghost, const int64_t global_pos[2],
                               const float origin[2], const float dX[2], int samples, const float background[4], int nregions,
                               const armon_region_f32* regions, float* rho, float* u, float* v, float* E)
{
    return init_regions_impl<float>(ctx, r, row_length, nghost, global_pos, origin, dX, samples, background, nregions, regions,
                                    rho, u, v, E);
}

int armon_hip_init_scalar_regions(armon_ctx* ctx, armon_range r, int64_t row_length, int nghost, const int64_t global_pos[2],
                                  const double origin[2], const double dX[2], int samples, const double background[4],
                                  int nregions, const armon_region* regions, double* phi, double* scratch_1, double* scratch_2,
                                  double* scratch_3)
{
    return init_regions_impl<double, armon_region, true>(ctx, r, row_length, nghost, global_pos, origin, dX, samples, background,
                                                         nregions, regions, phi, scratch_1, scratch_2, scratch_3);
}

int armon_hip_init_scalar_regions_f32(armon_ctx* ctx, armon_range r, int64_t row_length, int nghost, const int64_t global_pos[2],
                                      const float origin[2], const float dX[2], int samples, const float background[4],
                                      int nregions, const armon_region_f32* regions, float* phi, float* scratch_1,
                                      float* scratch_2, float* scratch_3)
{
    return init_regions_impl<float, armon_region_f32, true>(ctx, r, row_length, nghost, global_pos, origin, dX, samples, background,
                                                            nregions, regions, phi, scratch_1, scratch_2, scratch_3);
}

}  // extern "C"
