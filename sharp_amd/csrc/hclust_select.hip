// hclust_select.hip -- the host side of a5's last step (hclust.hip): which of the candidate levels a task takes, and the log of
// those decisions.  No kernel here.  select_level restates R/get_opt_hclust.R:162-229; it and decision_row have to agree line for
// line with the CPU checker of tests/ (its selection and its decision_row), whose log the tests compare with this one entry by entry.
#include "hclust_task.hpp"

#include <algorithm>
#include <limits>
#include <mutex>
#include <vector>

namespace sharp {

// model selection, R/get_opt_hclust.R:162-229
void select_level(const HcParams &prm, int n, int nk, const double *msil, const double *CH, const double *height,
                  int &oind, int &branch, int &rc) {
    double mx = msil[0];
    for (int c = 1; c < nk; ++c) if (msil[c] > mx) mx = msil[c];
    std::vector<int> ties;
    for (int c = 0; c < nk; ++c) if (msil[c] == mx) ties.push_back(c);
    oind = ties.empty() ? 1 : ties[(ties.size() + 1) / 2 - 1] + 1;   // tmp[ceiling(length(tmp)/2)]
    branch = 0;
    if (mx <= prm.sil_thre) {
        branch = 1;
        int wm = 0;
        for (int c = 1; c < nk; ++c) if (CH[c] > CH[wm]) wm = c;     // which.max: first maximum
        oind = wm + 1;
        if (oind == 1) {
            const int nh = n - 1, t0 = nh > 10 ? nh - 10 : 0, tl = nh - t0;
            const double *tmp = height + t0;
            int pind = -1;
            for (int i = 0; i + 1 < tl; ++i)
                if (tmp[i + 1] - tmp[i] > (prm.height_Ntimes - 1) * tmp[i]) { pind = i; break; }
            if (pind >= 0) {
                branch = 2;
                const double opth = (tmp[pind] + tmp[pind + 1]) / 2;
                int idx = n;                                         // which.max(c(height, Inf) > opth)
                for (int i = 0; i < n - 1; ++i) if (height[i] > opth) { idx = i + 1; break; }
                const int kk = n + 1 - idx;
                oind = kk - 1;                                       // "for consistency": assumes kmin == 2
            }
        }
    }
    if (oind < 1 || oind > nk) { rc |= SHARP_WARN_RANGE; oind = oind < 1 ? 1 : nk; }
}

// ---- the decision log (hclust.hpp) -------------------------------------------------------------------------------------------------
namespace {
struct DecisionLog { std::mutex mu; bool on = false; std::vector<double> rows; };
DecisionLog &dlog() { static DecisionLog *L = new DecisionLog; return *L; }
inline double dnan() { return std::numeric_limits<double>::quiet_NaN(); }
}  // namespace
bool decision_log_on() { return dlog().on || knobs().decision_log; }
void decision_log_set(bool on) { DecisionLog &L = dlog(); std::lock_guard<std::mutex> lk(L.mu); L.on = on; L.rows.clear(); }
void decision_log_add(const double *row) { DecisionLog &L = dlog(); std::lock_guard<std::mutex> lk(L.mu); L.rows.insert(L.rows.end(), row, row + kDecisionCols); }
void decision_log_override(int level, int block, int k_taken) {
    DecisionLog &L = dlog();
    std::lock_guard<std::mutex> lk(L.mu);
    for (size_t r = L.rows.size() / kDecisionCols; r-- > 0;) {        // (the latest row of that call)
        double *row = L.rows.data() + r * kDecisionCols;
        if (static_cast<int>(row[0]) == level && static_cast<int>(row[1]) == block) { row[12] = k_taken; return; }
    }
}
int decision_log_fetch(double *rows, int cap_rows) {
    DecisionLog &L = dlog();
    std::lock_guard<std::mutex> lk(L.mu);
    const int nr = static_cast<int>(L.rows.size() / kDecisionCols);
    std::vector<int> ord(nr);
    for (int i = 0; i < nr; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
        const double *x = L.rows.data() + static_cast<size_t>(a) * kDecisionCols, *y = L.rows.data() + static_cast<size_t>(b) * kDecisionCols;
        for (int c = 0; c < 4; ++c) if (x[c] != y[c]) return x[c] < y[c];
        return false;
    });
    for (int i = 0; i < nr && i < cap_rows; ++i)
        std::copy(L.rows.data() + static_cast<size_t>(ord[i]) * kDecisionCols, L.rows.data() + static_cast<size_t>(ord[i] + 1) * kDecisionCols,
                  rows + static_cast<size_t>(i) * kDecisionCols);
    return nr;
}
// the row of one decision: the same arithmetic, line for line, as the CPU checker's decision_row (the two logs are compared entry by entry)
void decision_row(const HcParams &prm, int n, int kmin, int nk, const double *msil, const double *CH, const double *height, int oind,
                  int branch, double *row) {
    for (int c = 0; c < kDecisionCols; ++c) row[c] = dnan();
    row[0] = prm.dec_level; row[1] = prm.dec_block; row[2] = prm.dec_k; row[3] = prm.dec_fold; row[4] = n;
    row[5] = branch; row[6] = kmin + oind - 1; row[12] = 0; row[13] = nk;
    if (prm.N_cluster > 0) { row[5] = 3; row[6] = prm.N_cluster; row[7] = 1; row[8] = msil[0]; row[13] = 1; return; }
    double mx = msil[0];
    for (int c = 1; c < nk; ++c) if (msil[c] > mx) mx = msil[c];
    row[10] = mx - prm.sil_thre;
    const double *val = branch == 0 ? msil : CH;
    double best = branch == 0 ? mx : val[0];
    if (branch != 0) for (int c = 1; c < nk; ++c) if (val[c] > best) best = val[c];
    int ties = 0;
    double second = dnan();
    for (int c = 0; c < nk; ++c) {
        if (val[c] == best) ++ties;
        else if (val[c] < best && (!(second == second) || val[c] > second)) second = val[c];
    }
    row[7] = ties; row[8] = best; row[9] = second;
    if (branch >= 1 && (branch == 2 || CH[0] == best)) {                    // which.max(CHind) == 1: the height rule was consulted (:196-210)
        bool first = true;
        for (int c = 1; c < nk; ++c) if (CH[c] > CH[0]) first = false;
        if (first) {
            const int nh = n - 1, t0 = nh > 10 ? nh - 10 : 0, tl = nh - t0;
            const double *tmp = height + t0;
            double rmax = dnan();
            for (int i = 0; i + 1 < tl; ++i) {
                const double dif = tmp[i + 1] - tmp[i], den = (prm.height_Ntimes - 1) * tmp[i];
                const double r = den > 0 ? dif / den : (dif > 0 ? std::numeric_limits<double>::infinity() : 0.0);
                if (branch == 2) { if (dif > den) { rmax = r; break; } }
                else if (!(rmax == rmax) || r > rmax) rmax = r;
            }
            row[11] = rmax;
        }
    }
}

// clusterCrit::intCriteria(., "Calinski_Harabasz") for the N.cluster-given branch (R/get_opt_hclust.R:105)
double host_ch_euclid(const double *y, int n, int p, const int *cl, int g) {
    std::vector<double> cen(static_cast<size_t>(g) * p, 0.0), all(p, 0.0);
    std::vector<int> cnt(g, 0);
    for (int i = 0; i < n; ++i) {
        const int c = cl[i] - 1; cnt[c]++;
        for (int k = 0; k < p; ++k) { cen[static_cast<size_t>(c) * p + k] += y[static_cast<size_t>(i) * p + k]; all[k] += y[static_cast<size_t>(i) * p + k]; }
    }
    for (int c = 0; c < g; ++c) for (int k = 0; k < p; ++k) cen[static_cast<size_t>(c) * p + k] /= cnt[c];
    for (int k = 0; k < p; ++k) all[k] /= n;
    double B = 0, W = 0;
    for (int c = 0; c < g; ++c) for (int k = 0; k < p; ++k) { const double d = cen[static_cast<size_t>(c) * p + k] - all[k]; B += cnt[c] * d * d; }
    for (int i = 0; i < n; ++i) for (int k = 0; k < p; ++k) { const double d = y[static_cast<size_t>(i) * p + k] - cen[static_cast<size_t>(cl[i] - 1) * p + k]; W += d * d; }
    return (B / (g - 1)) / (W / (n - g));
}

}  // namespace sharp
