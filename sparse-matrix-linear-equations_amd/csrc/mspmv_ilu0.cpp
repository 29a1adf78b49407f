// mspmv_ilu0.cpp -- ILU(0) preconditioner setup on the host, for the nonsymmetric solver
// (mspmv_dpbicgstab_ilu0_multi).  No reference counterpart: the reference has IC(0) only.
//
//   * L and U share A's pattern and A's CSR order: an entry with column < row holds L's multiplier
//     (unit diagonal implied), an entry with column >= row holds U;
//   * row by row in IKJ order: for each lower entry (i, k) of row i, ascending k,
//         l = w(k) / U(k,k);  w(k) = l;  w(j) -= l * U(k,j) for every j > k that both row i's and row
//     k's patterns hold (row k's upper part walked in CSR order);
//   * a zero or non-finite pivot U(i,i) is MSPMV_ERR_BREAKDOWN, naming the row.  No diagonal
//     shifting.
// Sequential host code, like mspmv_ic0_factor: setup, run once.  Compiled with -ffp-contract=off:
// every l * u and the subtraction after it round separately.  The four triangular solves it feeds run
// on the GPU every iteration (k_trsv_tagged, mspmv_tri.hip).
#include "mspmv_host.h"

#include <cmath>

using mspmv::invalid;

// Square, consistent offsets, columns in range; every row's columns strictly ascending (sorted, no
// duplicates) and holding the diagonal.  MSPMV_ERR_INVALID, the message naming the first offending
// row.  Shared by mspmv_ilu0_values, mspmv_color_greedy and the device factors' create calls (mspmv_tri.hip).
mspmv_status mspmv::ilu0_check_rows(const mspmv_csr_d *a, const char *who)
{
    const std::string w = std::string(who) + ": ";
    mspmv_status st = check_csr(a, who);
    if (st != MSPMV_OK)
        return st;
    if (a->num_rows != a->num_cols)
        return invalid(w + "ILU(0) needs a square matrix");
    const int n = a->num_rows;
    for (int i = 0; i < n; ++i) {
        int prev = -1;
        bool diag = false;
        for (int k = a->row_offsets[i]; k < a->row_offsets[i + 1]; ++k) {
            if (a->column_indices[k] <= prev)
                return invalid(w + "row " + std::to_string(i) + ": the columns must be strictly ascending");
            prev = a->column_indices[k];
            diag = diag || prev == i;
        }
        if (!diag)
            return invalid(w + "row " + std::to_string(i) + " has no diagonal entry");
    }
    return MSPMV_OK;
}

extern "C" MSPMV_API mspmv_status mspmv_ilu0_values(const mspmv_csr_d *a, double *lu_values)
{
    mspmv_status st = mspmv::ilu0_check_rows(a, "ilu0");
    if (st != MSPMV_OK)
        return st;
    if (a->num_nonzeros > 0 && !lu_values)
        return invalid("ilu0: null output");
    const int n = a->num_rows;
    const int *ro = a->row_offsets, *ci = a->column_indices;
    double *lu = lu_values;
    for (int k = 0; k < a->num_nonzeros; ++k)
        lu[k] = a->values[k];
    std::vector<int> diag((size_t)n, 0);  // position of U(i,i) in row i
    std::vector<int> pos((size_t)n, -1);  // column -> position in the row being factored
    for (int i = 0; i < n; ++i) {
        for (int k = ro[i]; k < ro[i + 1]; ++k) {
            pos[ci[k]] = k;
            if (ci[k] == i)
                diag[i] = k;
        }
        for (int ko = ro[i]; ko < diag[i]; ++ko) {
            const int k = ci[ko];
            const double l = lu[ko] / lu[diag[k]];  // row k's pivot passed its check
            lu[ko] = l;
            for (int jo = diag[k] + 1; jo < ro[k + 1]; ++jo) {
                const int p = pos[ci[jo]];
                if (p >= 0)
                    lu[p] = lu[p] - l * lu[jo];
            }
        }
        const double piv = lu[diag[i]];
        if (piv == 0.0 || !std::isfinite(piv)) {
            mspmv::set_error("ilu0: row " + std::to_string(i) + ": zero or non-finite pivot (no diagonal shifting)");
            return MSPMV_ERR_BREAKDOWN;
        }
        for (int k = ro[i]; k < ro[i + 1]; ++k)
            pos[ci[k]] = -1;
    }
    return MSPMV_OK;
}

void mspmv::split_lu(int n, const int *ro, const int *ci, const double *va, bool unit_diag, HostFactor &f)
{
    const size_t cap = (size_t)ro[n] + (unit_diag ? (size_t)n : 0);
    f.lro.assign((size_t)n + 1, 0), f.uro.assign((size_t)n + 1, 0);
    f.lci.clear(), f.lva.clear(), f.uci.clear(), f.uva.clear();
    f.lci.reserve(cap), f.lva.reserve(cap), f.uci.reserve(cap), f.uva.reserve(cap);
    for (int i = 0; i < n; ++i) {
        for (int k = ro[i]; k < ro[i + 1]; ++k) {
            if (ci[k] < i)
                f.lci.push_back(ci[k]), f.lva.push_back(va[k]);
            else  // the diagonal first: the columns ascend
                f.uci.push_back(ci[k]), f.uva.push_back(va[k]);
        }
        if (unit_diag)
            f.lci.push_back(i), f.lva.push_back(1.0);
        f.lro[(size_t)i + 1] = (int)f.lci.size();
        f.uro[(size_t)i + 1] = (int)f.uci.size();
    }
}
