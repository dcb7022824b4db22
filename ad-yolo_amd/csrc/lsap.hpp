// Rectangular linear sum assignment by shortest augmenting paths (Crouse, "On implementing 2D rectangular assignment
// algorithms", IEEE TAES 2016): the algorithm scipy.optimize.linear_sum_assignment runs, with the rules that decide which
// optimal assignment it returns when several exist:
//   * the problem is solved with rows <= columns (the caller transposes a tall matrix, as scipy does);
//   * the reduced path cost of column j from row i is  minVal + cost(i, j) - u[i] - v[j],  evaluated left to right in double;
//   * the remaining columns are scanned in the order of the `remaining` list, which starts as nc-1, nc-2, ..., 0; the column
//     taken leaves it by moving the last remaining column into its place;
//   * the scan keeps the first column of lowest path cost, except that a later UNASSIGNED column of equal cost replaces it.
// Only + - and comparisons touch the costs, so a faithful port picks the same assignment as scipy on bit-equal costs.
//
// Plain C++ (host) or HIP (device).  The column scans run lane-parallel: a context supplies lane(), width(), sync(), the
// cost and reduce(key, rank), a min-reduction over the lanes of (path cost, scan rank) pairs.  scan_rank() turns the
// sequential tie rule into a total order, so the reduction picks what the sequential scan picks.  With width() == 1 the
// code is the sequential algorithm.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LSAP_FN __host__ __device__ inline
#else
#define LSAP_FN inline
#endif

namespace lsap {

// Position `it` of the scan over nc columns -> rank (lower wins on equal path cost): an unassigned column beats every
// assigned one and the last unassigned one scanned wins; among assigned ones the first scanned wins.
LSAP_FN int scan_rank(int it, int nc, bool unassigned) { return unassigned ? nc - 1 - it : nc + it; }
LSAP_FN int scan_pos(int rank, int nc) { return rank < nc ? nc - 1 - rank : rank - nc; }
LSAP_FN bool better(double a, int ra, double b, int rb) { return a < b || (a == b && ra < rb); }

// Working arrays: u[nr], col4row[nr]; v, spc (shortest path costs), path, row4col, remaining, sc[nc].
struct State {
    double *u, *v, *spc;
    int *path, *col4row, *row4col, *remaining;
    unsigned char *sc;
};

// Solve an nr x nc problem with nr <= nc and nr <= 32.  On return col4row[i] is the column of row i and row4col[j] the row
// of column j (-1: none).  Returns 0, or -1 when no finite assignment exists (a NaN or infinite cost).
template <class Ctx>
LSAP_FN int solve(Ctx &cx, int nr, int nc, const State &s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int L = cx.lane(), W = cx.width();
    for (int i = L; i < nr; i += W) {
        s.u[i] = 0.0;
        s.col4row[i] = -1;
    }
    for (int j = L; j < nc; j += W) {
        s.v[j] = 0.0;
        s.row4col[j] = -1;
        s.path[j] = -1;
    }
    cx.sync();
    for (int cur = 0; cur < nr; ++cur) {
        for (int j = L; j < nc; j += W) {
            s.remaining[j] = nc - j - 1;
            s.sc[j] = 0;
            s.spc[j] = INFINITY;
        }
        cx.sync();
        uint32_t sr = 0;                                         // rows on the alternating tree
        double minv = 0.0;
        int nrem = nc, i = cur, sink = -1;
        while (sink < 0) {
            sr |= 1u << i;
            const double ui = s.u[i];
            double best = INFINITY;
            int brank = INT_MAX;
            for (int it = L; it < nrem; it += W) {
                const int j = s.remaining[it];
                const double r = minv + cx.cost(i, j) - ui - s.v[j];
                double sj = s.spc[j];
                if (r < sj) {
                    s.path[j] = i;
                    s.spc[j] = r;
                    sj = r;
                }
                const int rk = scan_rank(it, nc, s.row4col[j] < 0);
                if (better(sj, rk, best, brank)) {
                    best = sj;
                    brank = rk;
                }
            }
            cx.reduce(best, brank);
            if (brank == INT_MAX || !(best < INFINITY)) return -1;
            const int it = scan_pos(brank, nc);
            const int j = s.remaining[it];
            minv = best;
            const int owner = s.row4col[j];
            cx.sync();                                           // every lane has read remaining[] of this scan
            if (L == 0) {
                s.sc[j] = 1;
                s.remaining[it] = s.remaining[nrem - 1];
            }
            --nrem;
            if (owner < 0) sink = j;
            else i = owner;
            cx.sync();
        }
        if (L == 0) {
            s.u[cur] += minv;
            for (int r = 0; r < nr; ++r)
                if (((sr >> r) & 1u) && r != cur) s.u[r] += minv - s.spc[s.col4row[r]];
        }
        for (int j = L; j < nc; j += W)
            if (s.sc[j]) s.v[j] -= minv - s.spc[j];
        cx.sync();
        if (L == 0) {
            int j = sink;
            for (;;) {
                const int r = s.path[j];
                s.row4col[j] = r;
                const int t = s.col4row[r];
                s.col4row[r] = j;
                j = t;
                if (r == cur) break;
            }
        }
        cx.sync();
    }
    return 0;
}

// The column matched to row r of the ORIGINAL matrix (-1: none) after solve(); transposed: the solved problem had the
// original columns as its rows.  scipy returns exactly the rows with a match, ascending, with these columns.
LSAP_FN int match_of_row(const State &s, bool transposed, int r) { return transposed ? s.row4col[r] : s.col4row[r]; }

}  // namespace lsap
