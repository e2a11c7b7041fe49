// louvain.hpp -- Louvain community detection on a symmetric weighted graph: the project's own synchronous form of the
// method, built so that a call is a pure function of its arguments.  Weights are quantised to integers once (rule 1), so every sum of
// weights is an exact int64 sum whatever the order of the atomics; a round of local moving works from the round's start state and lets
// a community either lose or gain members (one hashed bit per community and round, rule 2); a round is kept when the modularity, summed
// in a fixed order, rises by more than tol (rule 3); the communities become the next level's vertices (rule 4).  The graph is what
// graph_source.hpp's fuzzy_graph_from_lists or snn_graph_from_lists leave on the device (graph.hpp's Graph), or any symmetric CSR.
// The C ABI entries (sharp_louvain_*, include/sharp_hip.h) wrap these.
#pragma once
#include <string>
#include <vector>

#include "graph.hpp"

namespace sharp {

// one level's graph on the device: integer weights, rows sorted by column, a self-loop entry holds a coarse vertex's internal weight
struct LouvainGraph : Csr<u64> {             // val: the integer weights q
    long long m2 = 0;                        // 2m = sum of k
    DevBuf<int> row;                         // nnz: the row of every entry
    DevBuf<u64> k;                           // n strengths
};

struct LouvainArgs {
    double resolution = 1.0, tol = 1e-7;
    int max_levels = 20, max_rounds = 200, max_fails = 4;
    unsigned long long seed = 10;
};

// what a level of Louvain or of Leiden (leiden.hpp) did; sub_communities and refine_rounds are Leiden's and stay 0 for Louvain
struct LouvainLevel {
    long long n = 0, communities = 0, sub_communities = 0;
    int rounds = 0, refine_rounds = 0;
    double q = 0.0;                          // of the level's accepted partition
};

// where a C ABI entry wants the levels (host, level_cap values each; membership: levels x n, or null).  sub_communities and
// refine_rounds are null in the Louvain entries.
struct LevelOut {
    long long *n, *communities, *sub_communities;
    int *rounds, *refine_rounds;
    double *q;
    int *n_levels, *membership;
    bool complete(bool leiden) const {
        return n && communities && rounds && q && n_levels && (!leiden || (sub_communities && refine_rounds));
    }
};

constexpr long long kLvMaxN = 1ll << 24;
constexpr long long kLvMaxNnz = 1ll << 38;
constexpr int kLvWaveCap = 128;              // rows up to this many entries: one wave, a 256-slot LDS table
constexpr int kLvBlockCap = 3072;            // up to this many: one workgroup, a 4096-slot LDS table; longer rows: a dense row in HBM

// the buffers of a level (sized for its n) and the row classes of its graph
struct LouvainWork {
    long long n = 0;
    DevBuf<u64> tot, tot2, in, scratch;
    DevBuf<int> present, pos;
    RowClasses rows;
    DevBuf<double> terms, sorted, part, out;
    Scratch tmp, tmp_sort;                   // (sized by the level's first lv_state, whose counts are its largest; reused by every round)
    bool sized = false;

    void size(long long nn);
    void classify(const LouvainGraph &L);
};

// rule 1 on a float-weighted graph; q = 0 entries are dropped from L
void louvain_quantise(const Graph &G, LouvainGraph &L);
// rules 2 - 5; membership: 1 .. G by decreasing size (host, n values); level_membership (when wanted): levels x n, the 0-based coarse
// vertex of every input vertex after each level
void louvain_run(LouvainGraph &L, const LouvainArgs &a, std::vector<int> &membership, std::vector<LouvainLevel> &levels,
                 std::vector<int> *level_membership);

// ---- the stages, for the methods built on them (Leiden, leiden.hip) -------------------------------------------------------------------
// k of L's entries
SHARP_LOCAL void lv_fill_strengths(LouvainGraph &L);
// tot, W.present / W.pos (the ranks of the surviving communities) and Q of the membership comm; returns Q and the number of communities.
// bound: a number the communities cannot exceed (0: n); only that many terms are sorted
SHARP_LOCAL double lv_state(const LouvainGraph &L, const int *comm, u64 *tot, LouvainWork &W, double gamma, long long *nc_out, long long bound = 0);
// prop = the proposals of one round (x1 = lv_round_key(seed, level, round)) from (comm, tot)
SHARP_LOCAL void lv_move(const LouvainGraph &L, const int *comm, const u64 *tot, LouvainWork &W, double gamma, u64 x1, int *prop);
// rules 2 and 3 from the membership in comm (n ids, device) to the level's end; spare: n ints.  The two pointers change places with
// every accepted round: on return comm is the accepted membership, its ranks are in W.pos.  Returns Q; rounds and the number of
// communities by pointer.
SHARP_LOCAL double lv_level(const LouvainGraph &L, const LouvainArgs &a, int lev, int *&comm, int *&spare, LouvainWork &W, int *rounds, long long *nc);
// the coarse graph of (L, comm) given the ranks W.pos of the surviving communities (lv_state of comm) and their number
SHARP_LOCAL void lv_aggregate(const LouvainGraph &L, const int *comm, const LouvainWork &W, long long nc, LouvainGraph &C);
// vmap[v] = W.pos[comm[vmap[v]]] for the n0 input vertices
SHARP_LOCAL void lv_compose(int *vmap, long long n0, const int *comm, const int *pos);
// 1 .. G by decreasing size, ties to the community with the smallest member; lab: ids in [0, nc)
SHARP_LOCAL void lv_relabel_by_size(const std::vector<int> &lab, long long nc, std::vector<int> &out);
// the checks and uploads of the C ABI entries (w: the entry's name for the messages)
SHARP_LOCAL void lv_check_csr_shape(const std::string &w, const long long *row_ptr, const int *col, long long n);
SHARP_LOCAL void lv_upload_float_graph(const std::string &w, const long long *row_ptr, const int *col, const double *val, long long n, Graph &G);
SHARP_LOCAL void lv_upload_int_graph(const std::string &w, const long long *row_ptr, const int *col, const long long *q, long long n, LouvainGraph &L);
SHARP_LOCAL void lv_upload_comm(const std::string &w, const int *comm, long long n, DevBuf<int> &d);
SHARP_LOCAL LouvainArgs louvain_args(const std::string &w, double resolution, double tol, int max_levels, int max_rounds, int max_fails, double seed);
// the shape of the neighbour lists that louvain_neighbors and leiden_neighbors take
SHARP_LOCAL void lv_check_list_shape(const std::string &w, long long n, int K);
// what the six sharp_{louvain,leiden}_{graph,neighbors,snn} entries do behind their graph: quantise G, run, refuse a level_cap below the
// number of levels, copy out.  modularity null (and max_refine_rounds 0): louvain_run; else leiden_run, which writes it.
SHARP_LOCAL void run_and_report(const std::string &w, const Graph &G, const LouvainArgs &a, int max_refine_rounds, int *membership,
                                double *modularity, int level_cap, const LevelOut &out);

}  // namespace sharp
