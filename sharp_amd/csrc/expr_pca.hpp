// expr_pca.hpp -- a truncated PCA of sparse expression blocks: the blocks on the device as a cell-major and a gene-major
// copy of the transformed values, the gene statistics, the two sparse x dense products, CholeskyQR2 and the fit.  The C ABI entries
// (sharp_expr_*, include/sharp_hip.h) are thin wrappers over these.
#pragma once
#include <string>
#include <vector>

#include "graph.hpp"

namespace sharp {

constexpr int kExprChunk = 512;                  // entries of a gene that one wave sums (the split rule of a per-destination sum pass)
constexpr int kExprSlabRows = 4096;              // rows of a slab of the l x l Gram
constexpr int kExprMaxL = 128;                   // n_components + oversample: two columns per lane
constexpr long long kExprMaxN = 2147483646ll;
constexpr int kExprMaxM = 16777216;
constexpr long long kExprMaxNnz = 1ll << 38;

// a list of CSC blocks as the C ABI hands it over: colptr[b] (ncb[b] + 1 ints), rowidx[b] (0-based genes), val[b]
struct ExprBlocks {
    const int *const *colptr;
    const int *const *rowidx;
    const double *const *val;
    const long long *ncb;
    int nblocks, m;
};

// what expr_load does beyond §21's options
struct ExprExtra {
    const int *genes = nullptr;                  // keep these genes (strictly ascending, within [0, m)), renumbered by their position
    int n_genes = 0;                             // (nullptr and 0: all genes)
    bool refuse_negative = false;                // raw counts are expected: a negative value is refused without a transform too
    bool want_tsum = false;                      // the cells' sums of the transformed values over all genes, into ExprData::tsum
};

struct ExprData {
    long long n = 0, nnz = 0, nch = 0;
    int m = 0;                                   // the genes of the copies below: the kept ones under a subset
    int m_in = 0;                                // the genes of the blocks
    DevBuf<long long> cptr;                      // n + 1: a cell's entries
    DevBuf<int> ridx;                            // nnz: their genes, ascending within a cell
    DevBuf<double> t;                            // nnz: the transformed values
    DevBuf<double> lsum;                         // n: the cells' sums before the transform, over all genes
    DevBuf<double> tsum;                         // n: the cells' sums after it, over all genes (ExprExtra::want_tsum)
    DevBuf<long long> gptr;                      // m + 1: a gene's entries in the gene-major copy
    DevBuf<int> gcell;                           // nnz: their cells, ascending within a gene
    DevBuf<double> gval;                         // nnz
    DevBuf<long long> chptr;                     // m + 1: a gene's chunks of kExprChunk entries
    DevBuf<int> chgene;                          // nch: the gene of a chunk
    DevBuf<double> mu, var, sd, w;               // m each: mean, variance, the result's `scale`, the weight
    DevBuf<long long> gnnz;                      // m: the non-zero values of a gene
    double total_var = 0.0;
};

// validates and uploads the blocks, transforms the values; genes: also the gene-major copy, the chunks and the statistics (scale: w = 1 /
// sd).  l_work: the columns of the dense workspaces the caller will hold, for the refusal before anything is allocated.
// extra.genes: the entries of the other genes are dropped after the transform (the cells' sums L_c are over all genes) and before the
// gene-major copy is built; from there on D.m = extra.n_genes.
void expr_load(const std::string &who, const ExprBlocks &B, double normalize_total, bool log1p, bool genes, bool scale, int l_work,
               long long min_cells, ExprData &D, const ExprExtra &extra = ExprExtra());
// two steps of expr_load for a caller that made the cell-major copy itself (doublets.hip: D.cptr, D.ridx, D.t, D.lsum, D.n, D.m, D.nnz):
// the transform of the values in place, and the drop of the genes that `genes` (checked by expr_check_genes) does not keep
void expr_transform(ExprData &D, double normalize_total, bool log1p);
void expr_subset(ExprData &D, const int *genes, int n_genes);
// the genes kept of m: n_genes when `genes` is a strictly ascending list within [0, m), m for (nullptr, 0); anything else is refused by name
int expr_check_genes(const std::string &who, const int *genes, int n_genes, int m);
// the checks of the options and of the block list that need no device; the second returns the cells in all
void expr_check_options(const std::string &who, double normalize_total, int m);
long long expr_total_cells(const std::string &who, const ExprBlocks &B);
// Y (n x l) = A Bm, Bm m x l on the device: Y[c, :] = sum over the cell's entries of t_gc w_g Bm[g, :] - mu^T diag(w) Bm
void expr_spmm_cells(const ExprData &D, const double *mu, const double *w, const double *Bm, int l, double *Y);
// Z (m x l) = A^T Q, Q n x l on the device
void expr_spmm_genes(const ExprData &D, const double *Q, int l, double *Z);
// Y (rows x l, device) -> Q with orthonormal columns, in place (CholeskyQR2)
void expr_orth(const std::string &who, double *Y, long long rows, int l);


// the entries [b, e) of chunk ch of gene g
__device__ __forceinline__ void chunk_range(const long long *__restrict__ gptr, const long long *__restrict__ chptr, int g, long long ch,
                                            long long &b, long long &e) {
    b = gptr[g] + (ch - chptr[g]) * kExprChunk;
    const long long ge = gptr[g + 1];
    e = b + kExprChunk < ge ? b + kExprChunk : ge;
}

unsigned wave_grid(long long items);             // workgroups of four waves, one item per wave

}  // namespace sharp
