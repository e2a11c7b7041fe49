// umap_transform.hip -- new rows placed in a fitted UMAP map: DESIGN.md §14 (the project's specification, modelled on umap-learn's
// transform and uwot's umap_transform; no bit parity with either is claimed).
//   model      a device-resident handle: the reference rows X_ref, their column mean mu, W = X_ref - mu, ||w_j||^2, the fitted map
//              Y_ref, a, b, n_neighbors and the fit's n_epochs
//   lists      the K nearest reference rows of every query row: knn.hip's cross search
//   weights    one wave per row: sigma by §13's bisection with rho = 0, the floor on the row's own mean, w = exp(-d / sigma), and the
//              start y = sum w Y_ref[idx] / sum w
//   epochs     one wave per row, lanes over the slots p * T + term; Y_ref is fixed and rows are independent, so the kernel runs the
//              epochs [ep0, ep1) itself with y in registers: one launch for the whole range
// A row's result depends on (the row, the model, the arguments, row_offset + q) alone: not on the rows beside it, the launch split or
// the candidate chunking.  fp64 throughout, no floating-point atomics, every sum in an order fixed by the shape.
#include "knn.hpp"
#include "umap.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace sharp {
namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// weights and start
// ---------------------------------------------------------------------------------------------------------------------------
// One wave per query row (four 64-wide strides of registers, K <= 255): §13's bisection with rho = 0 (lo = 0, hi = inf, mid = 1, at most
// 64 steps, tolerance 1e-5 on the sum), sigma = max(mid, 1e-3 * the row's own mean distance), w = exp(-d / sigma), and the start
// y = sum_j w_j Y_ref[idx_j] / sum_j w_j.  Every sum runs per lane over its strides, then the butterfly.  A row whose weights all
// underflow (K = 1 and a distance beyond 745: exp(-d) = 0 meets log2 1 at once) starts at its nearest reference row's position.
template <int DIMS>
__global__ __launch_bounds__(256) void transform_weight_kernel(const int *__restrict__ idx, const double *__restrict__ dist, long long nq, int K,
                                                               double target, const double *__restrict__ Yref, double *__restrict__ sigma,
                                                               double *__restrict__ w, double *__restrict__ Y0) {
    const int lane = threadIdx.x & 63;
    const long long q = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    double dv[4], rs = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = lane + 64 * t;
        dv[t] = p < K ? dist[q * K + p] : 0.0;
        rs += dv[t];
    }
    rs = wave_sum(rs);
    double lo = 0.0, hi = HUGE_VAL, mid = 1.0;
    for (int it = 0; it < 64; ++it) {
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (lane + 64 * t < K) s += exp(-dv[t] / mid);
        s = wave_sum(s);
        if (fabs(s - target) < 1e-5) break;
        if (s > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == HUGE_VAL ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double sg = fmax(mid, 1e-3 * (rs / static_cast<double>(K)));
    if (lane == 0) sigma[q] = sg;
    double sw = 0.0, sy[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) sy[k] = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = lane + 64 * t;
        if (p >= K) continue;
        const double wv = exp(-dv[t] / sg);
        w[q * K + p] = wv;
        sw += wv;
        const long long j = idx[q * K + p];
#pragma unroll
        for (int k = 0; k < DIMS; ++k) sy[k] += wv * Yref[j * DIMS + k];
    }
    sw = wave_sum(sw);
#pragma unroll
    for (int k = 0; k < DIMS; ++k) sy[k] = wave_sum(sy[k]);
    if (lane == 0) {
        const long long j0 = idx[q * K];
#pragma unroll
        for (int k = 0; k < DIMS; ++k) Y0[q * DIMS + k] = sw > 0.0 ? sy[k] / sw : Yref[j0 * DIMS + k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// epochs
// ---------------------------------------------------------------------------------------------------------------------------
// One wave per query row q, lanes over the slots s = p * T + term of the row (T = 1 + negative_sample_rate), pass after pass of 64 in
// slot order, for the epochs [ep0, ep1) of E one after the other with y_q in registers (the butterfly leaves every lane the same sum, so
// every lane carries the same y).  Slot p's rate is w_qp; its edge number, for the draw, is (row_offset + q) K + p.  No factor 2 on the
// attraction and no self test on the drawn vertex: a query is not a reference row.  Y_ref is only read.
template <int DIMS>
__global__ __launch_bounds__(256) void transform_epoch_kernel(const int *__restrict__ idx, const double *__restrict__ w, long long nq, int K,
                                                              const double *__restrict__ Yref, long long nref, double *__restrict__ Yq, int E,
                                                              int ep0, int ep1, double learning_rate, double a, double b, double gamma, int T,
                                                              unsigned long long seed, long long row_offset) {
    const int lane = threadIdx.x & 63;
    const long long q = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    double y[DIMS];
#pragma unroll
    for (int k = 0; k < DIMS; ++k) y[k] = Yq[q * DIMS + k];
    const unsigned slots = static_cast<unsigned>(K) * static_cast<unsigned>(T);   // (<= 255 * 65)
    const unsigned long long e0 = static_cast<unsigned long long>(row_offset + q) * static_cast<unsigned long long>(K);
    for (int ep = ep0 > 1 ? ep0 : 1; ep < ep1; ++ep) {   // (nothing fires in epoch 0)
        const double alpha = learning_rate * (1.0 - static_cast<double>(ep) / static_cast<double>(E));
        const unsigned long long x0 = mix64(seed * 0x9E3779B97F4A7C15ull + static_cast<unsigned long long>(ep));
        const double epd = static_cast<double>(ep), epm = static_cast<double>(ep - 1);
        double acc[DIMS];
#pragma unroll
        for (int k = 0; k < DIMS; ++k) acc[k] = 0.0;
        for (unsigned s = lane; s < slots; s += 64) {
            const unsigned p = s / static_cast<unsigned>(T), t = s - p * static_cast<unsigned>(T);
            const double r = w[q * K + p];
            if (!(floor(epd * r) > floor(epm * r))) continue;
            long long v;
            if (t == 0) {
                v = idx[q * K + p];
            } else {
                const unsigned long long x = mix64(mix64(x0 + e0 + p) + static_cast<unsigned long long>(t - 1));
                v = static_cast<long long>(floor(static_cast<double>(x >> 11) * 0x1.0p-53 * static_cast<double>(nref)));
                if (v > nref - 1) v = nref - 1;   // (never taken: (1 - 2^-53) n rounds below n)
            }
            double diff[DIMS], D = 0.0;
#pragma unroll
            for (int k = 0; k < DIMS; ++k) { diff[k] = y[k] - Yref[v * DIMS + k]; D += diff[k] * diff[k]; }
            if (!(D > 0.0)) continue;
            const double den = a * pow(D, b) + 1.0;
            const double c = t == 0 ? (-2.0 * a * b * pow(D, b - 1.0)) / den : (2.0 * gamma * b) / ((0.001 + D) * den);
#pragma unroll
            for (int k = 0; k < DIMS; ++k) acc[k] += clip4(c * diff[k]);
        }
#pragma unroll
        for (int k = 0; k < DIMS; ++k) y[k] = y[k] + alpha * wave_sum(acc[k]);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DIMS; ++k) Yq[q * DIMS + k] = y[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the model and its registry
// ---------------------------------------------------------------------------------------------------------------------------
struct UmapModel {
    int slot = 0;                 // the context that made it
    long long n = 0;
    int d = 0, dims = 0, n_neighbors = 0, n_epochs = 0;
    double a = 0.0, b = 0.0;
    DevBuf<double> X, W, wn, mu, Y;   // n x d, n x d, n, d, n x dims
};

std::mutex g_mu;
std::map<int, std::shared_ptr<UmapModel>> g_models;
int g_next = 1;

std::shared_ptr<UmapModel> get_model(int handle, const char *who) {
    std::shared_ptr<UmapModel> m;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_models.find(handle);
        if (it != g_models.end()) m = it->second;
    }
    SHARP_REQUIRE(m, std::string(who) + ": handle is not a live UMAP model (freed, or never created)");
    SHARP_REQUIRE(m->slot == cur_slot(), std::string(who) + ": handle belongs to another device context");
    return m;
}

// rows of a host matrix (row i at X + i * ld) packed on the device, refused by name when a value is not finite
void upload_checked(const double *X, long long n, int d, long long ld, const std::string &who, const char *arg, DevBuf<double> &dst) {
    for (long long i = 0; i < n; ++i)
        for (int c = 0; c < d; ++c)
            if (!std::isfinite(X[i * ld + c]))
                throw Error(SHARP_ERR_ARG, who + ": " + arg + " holds NA / NaN / Inf (row " + std::to_string(i + 1) + ", column " +
                                               std::to_string(c + 1) + ")");
    upload_rows(X, n, d, ld, dst);
    stream_sync();
}

void check_run_args(const char *who, int E, int ep0, int ep1, double learning_rate, int negative_sample_rate, double repulsion_strength,
                    double seed, long long row_offset, long long nq, int K) {
    const std::string w(who);
    SHARP_REQUIRE(E >= 0 && ep0 >= 0 && ep0 <= ep1 && ep1 <= E, w + ": need 0 <= ep0 <= ep1 <= n_epochs");
    SHARP_REQUIRE(std::isfinite(learning_rate), w + ": learning_rate must be finite");
    SHARP_REQUIRE(negative_sample_rate >= 0 && negative_sample_rate <= 64, w + ": negative_sample_rate must be in 0 .. 64");
    SHARP_REQUIRE(std::isfinite(repulsion_strength), w + ": repulsion_strength must be finite");
    SHARP_REQUIRE(std::isfinite(seed) && std::fabs(seed) < 9.0e18, w + ": seed must be a finite integer");
    SHARP_REQUIRE(row_offset >= 0, w + ": row_offset must be >= 0");
    // (row_offset + nq) K T < 2^63 with K T <= 255 * 65 < 2^15
    SHARP_REQUIRE(row_offset <= (1ll << 47) && nq <= (1ll << 47), w + ": row_offset + nq must stay below 2^48 (the edge numbers are 64-bit)");
    (void)K;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// the stages on device buffers
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

void transform_weights(const UmapModel &m, const int *idx, const double *dist, long long nq, int K, double *sigma, double *w, double *Y0) {
    Ctx &c = ctx();
    KernelTimer t("umap_tr_weights");
    const double target = std::log2(static_cast<double>(K));
    const dim3 grid(grid_for(nq, 4)), block(256);
    if (m.dims == 1)
        hipLaunchKernelGGL(transform_weight_kernel<1>, grid, block, 0, c.stream, idx, dist, nq, K, target, m.Y.p, sigma, w, Y0);
    else if (m.dims == 2)
        hipLaunchKernelGGL(transform_weight_kernel<2>, grid, block, 0, c.stream, idx, dist, nq, K, target, m.Y.p, sigma, w, Y0);
    else
        hipLaunchKernelGGL(transform_weight_kernel<3>, grid, block, 0, c.stream, idx, dist, nq, K, target, m.Y.p, sigma, w, Y0);
    launch_check("transform_weight_kernel");
}

void transform_epochs(const UmapModel &m, const int *idx, const double *w, long long nq, int K, double *Yq, int E, int ep0, int ep1,
                      double learning_rate, int negative_sample_rate, double repulsion_strength, unsigned long long seed, long long row_offset) {
    Ctx &c = ctx();
    if (ep0 == ep1) return;
    KernelTimer t("umap_tr_epochs");
    const int T = 1 + negative_sample_rate;
    const dim3 grid(grid_for(nq, 4)), block(256);
    if (m.dims == 1)
        hipLaunchKernelGGL(transform_epoch_kernel<1>, grid, block, 0, c.stream, idx, w, nq, K, m.Y.p, m.n, Yq, E, ep0, ep1, learning_rate, m.a, m.b,
                           repulsion_strength, T, seed, row_offset);
    else if (m.dims == 2)
        hipLaunchKernelGGL(transform_epoch_kernel<2>, grid, block, 0, c.stream, idx, w, nq, K, m.Y.p, m.n, Yq, E, ep0, ep1, learning_rate, m.a, m.b,
                           repulsion_strength, T, seed, row_offset);
    else
        hipLaunchKernelGGL(transform_epoch_kernel<3>, grid, block, 0, c.stream, idx, w, nq, K, m.Y.p, m.n, Yq, E, ep0, ep1, learning_rate, m.a, m.b,
                           repulsion_strength, T, seed, row_offset);
    launch_check("transform_epoch_kernel");
}

// a caller's lists for the stage entries: every index inside the reference
void check_stage_lists(const std::string &who, const UmapModel &m, const int *idx, long long nq, int K) {
    SHARP_REQUIRE(nq >= 1 && nq < INT_MAX, who + ": nq must be in 1 .. 2^31 - 1");
    SHARP_REQUIRE(K >= 1 && K <= 255, who + ": K must be in 1 .. 255");
    for (long long e = 0; e < nq * K; ++e)
        if (idx[e] < 0 || idx[e] >= m.n)
            throw Error(SHARP_ERR_ARG, who + ": idx holds an index outside the reference (row " + std::to_string(e / K) + ")");
}

}  // namespace

void umap_models_drop_slot(int slot) {
    std::vector<std::shared_ptr<UmapModel>> gone;   // (freed outside the registry lock)
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto it = g_models.begin(); it != g_models.end();)
        if (it->second->slot == slot) { gone.push_back(std::move(it->second)); it = g_models.erase(it); } else ++it;
}

}  // namespace sharp

using namespace sharp;

extern "C" {

int sharp_umap_model_create(const double *X_ref, long long n_ref, int d, long long ld, const double *Y_ref, int dims, int n_neighbors, double a,
                            double b, int n_epochs, int *handle) {
    SHARP_API_BEGIN
    ctx();
    const std::string who = "sharp_umap_model_create";
    SHARP_REQUIRE(handle, who + ": null handle");
    SHARP_REQUIRE(X_ref && n_ref >= 1 && n_ref < INT_MAX && d >= 1 && ld >= d, who + ": bad X_ref (need 1 <= n_ref < 2^31 rows of d >= 1 values, ld >= d)");
    SHARP_REQUIRE(Y_ref, who + ": null Y_ref");
    SHARP_REQUIRE(dims >= 1 && dims <= 3, who + ": dims must be 1, 2 or 3");
    SHARP_REQUIRE(n_neighbors >= 1 && n_neighbors <= 255, who + ": n_neighbors must be in 1 .. 255");
    SHARP_REQUIRE(n_neighbors <= n_ref, who + ": n_neighbors must not exceed n_ref");
    SHARP_REQUIRE(std::isfinite(a) && std::isfinite(b) && a > 0.0 && b > 0.0, who + ": a and b must be positive");
    SHARP_REQUIRE(n_epochs >= 0, who + ": n_epochs must be >= 0");
    auto m = std::make_shared<UmapModel>();
    m->slot = cur_slot();
    m->n = n_ref;
    m->d = d;
    m->dims = dims;
    m->n_neighbors = n_neighbors;
    m->n_epochs = n_epochs;
    m->a = a;
    m->b = b;
    upload_checked(X_ref, n_ref, d, ld, who, "X_ref", m->X);
    upload_checked(Y_ref, n_ref, dims, dims, who, "Y_ref", m->Y);
    std::vector<double> mu(d, 0.0);   // the column mean: row after row, one division
    for (long long i = 0; i < n_ref; ++i)
        for (int c = 0; c < d; ++c) mu[c] += X_ref[i * ld + c];
    for (int c = 0; c < d; ++c) mu[c] /= static_cast<double>(n_ref);
    m->mu.alloc(d);
    m->mu.upload(mu.data(), d);
    center_and_norm(m->X.p, n_ref, d, m->mu.p, m->W, m->wn, who + ": X_ref holds values so large that squared distances overflow");
    {
        std::lock_guard<std::mutex> lk(g_mu);
        *handle = g_next++;
        g_models[*handle] = std::move(m);
    }
    SHARP_API_END
}

int sharp_umap_model_free(int handle) {
    SHARP_API_BEGIN
    ctx();
    auto m = get_model(handle, "sharp_umap_model_free");
    stream_sync();
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_models.erase(handle);
    }
    SHARP_API_END
}

int sharp_knn_cross(int handle, const double *Xq, long long nq, long long ld, int K, int max_rows_per_launch, int *idx, double *dist) {
    SHARP_API_BEGIN
    ctx();
    const char *who = "sharp_knn_cross";
    auto m = get_model(handle, who);
    SHARP_REQUIRE(Xq && idx && dist, std::string(who) + ": null Xq / idx / dist");
    SHARP_REQUIRE(nq >= 1 && nq < INT_MAX && ld >= m->d, std::string(who) + ": need 1 <= nq < 2^31 rows and ld >= the model's d");
    DevBuf<double> dXq, dd;
    DevBuf<int> di;
    upload_checked(Xq, nq, m->d, ld, who, "Xq", dXq);
    knn_cross(who, m->W.p, m->wn.p, m->X.p, m->mu.p, m->n, m->d, dXq.p, nq, K, max_rows_per_launch, di, dd);
    di.download(idx, static_cast<size_t>(nq) * K);
    dd.download(dist, static_cast<size_t>(nq) * K);
    SHARP_API_END
}

int sharp_umap_transform_weights(int handle, const int *idx, const double *dist, long long nq, int K, double *sigma, double *w, double *Y0) {
    SHARP_API_BEGIN
    ctx();
    const std::string who = "sharp_umap_transform_weights";
    auto m = get_model(handle, who.c_str());
    SHARP_REQUIRE(idx && dist && sigma && w && Y0, who + ": null argument");
    check_stage_lists(who, *m, idx, nq, K);
    const size_t ne = static_cast<size_t>(nq) * K;
    for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(dist[e] >= 0.0 && dist[e] <= DBL_MAX, who + ": dist holds a value that is NA / NaN / Inf or negative");
    DevBuf<int> di(ne);
    DevBuf<double> dd(ne), ds(nq), dw(ne), dy(static_cast<size_t>(nq) * m->dims);
    di.upload(idx, ne);
    dd.upload(dist, ne);
    transform_weights(*m, di.p, dd.p, nq, K, ds.p, dw.p, dy.p);
    ds.download(sigma, nq);
    dw.download(w, ne);
    dy.download(Y0, static_cast<size_t>(nq) * m->dims);
    SHARP_API_END
}

int sharp_umap_transform_epochs(int handle, const int *idx, const double *w, long long nq, int K, double *Yq, int n_epochs, int ep0, int ep1,
                                double learning_rate, int negative_sample_rate, double repulsion_strength, double seed, long long row_offset) {
    SHARP_API_BEGIN
    ctx();
    const std::string who = "sharp_umap_transform_epochs";
    auto m = get_model(handle, who.c_str());
    SHARP_REQUIRE(idx && w && Yq, who + ": null argument");
    check_stage_lists(who, *m, idx, nq, K);
    check_run_args(who.c_str(), n_epochs, ep0, ep1, learning_rate, negative_sample_rate, repulsion_strength, seed, row_offset, nq, K);
    const size_t ne = static_cast<size_t>(nq) * K, ny = static_cast<size_t>(nq) * m->dims;
    for (size_t e = 0; e < ne; ++e) SHARP_REQUIRE(w[e] >= 0.0 && w[e] <= 1.0, who + ": w holds a weight outside [0, 1] (or NA / NaN)");
    for (size_t e = 0; e < ny; ++e) SHARP_REQUIRE(std::isfinite(Yq[e]), who + ": Yq holds NA / NaN / Inf");
    DevBuf<int> di(ne);
    DevBuf<double> dw(ne), dy(ny);
    di.upload(idx, ne);
    dw.upload(w, ne);
    dy.upload(Yq, ny);
    transform_epochs(*m, di.p, dw.p, nq, K, dy.p, n_epochs, ep0, ep1, learning_rate, negative_sample_rate, repulsion_strength,
                     static_cast<unsigned long long>(static_cast<long long>(seed)), row_offset);
    dy.download(Yq, ny);
    SHARP_API_END
}

int sharp_umap_transform(int handle, const double *Xq, long long nq, long long ld, int n_epochs, double learning_rate, int negative_sample_rate,
                         double repulsion_strength, double seed, long long row_offset, double *Yq, int *nn_index, double *nn_distance) {
    SHARP_API_BEGIN
    ctx();
    const std::string who = "sharp_umap_transform";
    auto m = get_model(handle, who.c_str());
    SHARP_REQUIRE(Xq && Yq, who + ": null Xq / Yq");
    SHARP_REQUIRE(nq >= 1 && nq < INT_MAX && ld >= m->d, who + ": need 1 <= nq < 2^31 rows and ld >= the model's d");
    SHARP_REQUIRE((nn_index == nullptr) == (nn_distance == nullptr), who + ": nn_index and nn_distance go together");
    const int E = n_epochs >= 0 ? n_epochs : m->n_epochs / 3;
    check_run_args(who.c_str(), E, 0, E, learning_rate, negative_sample_rate, repulsion_strength, seed, row_offset, nq, m->n_neighbors);
    const int K = m->n_neighbors;
    DevBuf<double> dXq, dist;
    DevBuf<int> idx;
    upload_checked(Xq, nq, m->d, ld, who, "Xq", dXq);
    knn_cross(who.c_str(), m->W.p, m->wn.p, m->X.p, m->mu.p, m->n, m->d, dXq.p, nq, K, 0, idx, dist);
    dXq.release();
    if (nn_index) {
        idx.download(nn_index, static_cast<size_t>(nq) * K);
        dist.download(nn_distance, static_cast<size_t>(nq) * K);
    }
    const size_t ny = static_cast<size_t>(nq) * m->dims;
    DevBuf<double> sigma(nq), w(static_cast<size_t>(nq) * K), dy(ny);
    transform_weights(*m, idx.p, dist.p, nq, K, sigma.p, w.p, dy.p);
    transform_epochs(*m, idx.p, w.p, nq, K, dy.p, E, 0, E, learning_rate, negative_sample_rate, repulsion_strength,
                     static_cast<unsigned long long>(static_cast<long long>(seed)), row_offset);
    dy.download(Yq, ny);
    SHARP_API_END
}

}  // extern "C"
