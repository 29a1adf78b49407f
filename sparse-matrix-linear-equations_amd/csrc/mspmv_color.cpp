// mspmv_color.cpp -- multi-colour ordering for ILU(0) and IC(0), on the host (mspmv_ilu0_create_colored,
// mspmv_ic0_create_colored).  No reference counterpart.
//
//   * mspmv_color_greedy: rows 0..n-1 in turn take the smallest colour no already-coloured neighbour holds, the
//     neighbours being those of A + A^T's off-diagonal pattern (stored zeros count).  Sequential, deterministic.
//   * mspmv_csr_permute_sym: Ap = P A P^T, row i of Ap being row perm[i] of A, every row's columns ascending.
//   * ilu0_colored_host: colours (given or greedy) -> perm (rows stably sorted by colour) -> Ap -> ILU(0) of Ap by
//     mspmv_ilu0_values -> L (strictly lower, unit diagonal implied) and U (diagonal first).  Rows of one colour
//     share no entry, so row i of L reads only rows of earlier colours and row i of U only rows of later ones: a
//     colour is one independent sweep (k_trsv_color, mspmv_color.hip), the factor has at most C levels.
//   * ic0_colored_host: the same colours, perm and Ap (color_order, shared) -> mspmv_ic0_factor of Ap, diagonal
//     shifts included -> L (diagonal last) and L^T by mspmv_csr_transpose (diagonal first).
// Everything here runs before the device is touched.
#include "mspmv_host.h"

#include <algorithm>
#include <utility>

using mspmv::HostFactor;
using mspmv::invalid;

// colors[i] for a matrix that passed ilu0_check_rows; returns the number of colours
static int greedy(const mspmv_csr_d *a, int *colors)
{
    const int n = a->num_rows;
    const int *ro = a->row_offsets, *ci = a->column_indices;
    // A^T's pattern by counting sort: tci[tro[j] .. tro[j+1]) = the rows that hold column j
    std::vector<int> tro((size_t)n + 1, 0), tci((size_t)std::max(a->num_nonzeros, 1));
    for (int k = 0; k < a->num_nonzeros; ++k)
        ++tro[(size_t)ci[k] + 1];
    for (int j = 0; j < n; ++j)
        tro[(size_t)j + 1] += tro[j];
    {
        std::vector<int> pos(tro.begin(), tro.end() - 1);
        for (int i = 0; i < n; ++i)
            for (int k = ro[i]; k < ro[i + 1]; ++k)
                tci[(size_t)pos[ci[k]]++] = i;
    }
    std::vector<int> held((size_t)n + 1, -1);  // held[c] == i: a coloured neighbour of row i holds colour c
    int num = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = ro[i]; k < ro[i + 1]; ++k)
            if (ci[k] < i)
                held[colors[ci[k]]] = i;
        for (int k = tro[i]; k < tro[i + 1]; ++k)
            if (tci[k] < i)
                held[colors[tci[k]]] = i;
        int c = 0;
        while (held[c] == i)
            ++c;
        colors[i] = c;
        num = std::max(num, c + 1);
    }
    return num;
}

extern "C" MSPMV_API mspmv_status mspmv_color_greedy(const mspmv_csr_d *a, int *colors, int *num_colors)
{
    mspmv_status st = mspmv::ilu0_check_rows(a, "color_greedy");
    if (st != MSPMV_OK)
        return st;
    if ((a->num_rows > 0 && !colors) || !num_colors)
        return invalid("color_greedy: null output");
    *num_colors = greedy(a, colors);
    return MSPMV_OK;
}

// Ap = P A P^T into ro [n + 1], ci, va [nnz]; a: square with consistent offsets and columns in range
static void permute(const mspmv_csr_d *a, const int *perm, const std::vector<int> &inv, int *ro, int *ci, double *va)
{
    const int n = a->num_rows;
    std::vector<std::pair<int, double>> row;
    ro[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int r = perm[i];
        row.clear();
        for (int k = a->row_offsets[r]; k < a->row_offsets[r + 1]; ++k)
            row.emplace_back(inv[a->column_indices[k]], a->values[k]);
        std::stable_sort(row.begin(), row.end(),
                         [](const std::pair<int, double> &x, const std::pair<int, double> &y) { return x.first < y.first; });
        int o = ro[i];
        for (const auto &e : row) {
            ci[o] = e.first;
            va[o++] = e.second;
        }
        ro[i + 1] = o;
    }
}

static mspmv_status inverse_perm(int n, const int *perm, std::vector<int> &inv, const char *who)
{
    inv.assign((size_t)n, -1);
    for (int i = 0; i < n; ++i) {
        if (perm[i] < 0 || perm[i] >= n)
            return invalid(std::string(who) + ": perm[" + std::to_string(i) + "] is out of range");
        if (inv[perm[i]] >= 0)
            return invalid(std::string(who) + ": perm[" + std::to_string(i) + "] repeats an index");
        inv[perm[i]] = i;
    }
    return MSPMV_OK;
}

extern "C" MSPMV_API mspmv_status mspmv_csr_permute_sym(const mspmv_csr_d *a, const int *perm, int *ro, int *ci,
                                                        double *va)
{
    const char *who = "csr_permute_sym";
    mspmv_status st = mspmv::check_csr(a, who);
    if (st != MSPMV_OK)
        return st;
    if (a->num_rows != a->num_cols)
        return invalid(std::string(who) + ": a symmetric permutation needs a square matrix");
    const int n = a->num_rows;
    if (!ro || (n > 0 && !perm) || (a->num_nonzeros > 0 && (!ci || !va)))
        return invalid(std::string(who) + ": null permutation or output");
    std::vector<int> inv;
    st = inverse_perm(n, perm, inv, who);
    if (st != MSPMV_OK)
        return st;
    permute(a, perm, inv, ro, ci, va);
    return MSPMV_OK;
}

// Colours (given and checked, or greedy) -> perm (rows stably sorted by colour) -> Ap = P A P^T into pro, pci, pva.
// a: square with consistent offsets and columns in range; who prefixes the messages.
static mspmv_status color_order(const mspmv_csr_d *a, const int *colors, const char *who, std::vector<int> &perm,
                                std::vector<int> &color_off, std::vector<int> &pro, std::vector<int> &pci,
                                std::vector<double> &pva)
{
    const int n = a->num_rows, nnz = a->num_nonzeros;
    std::vector<int> col((size_t)n, 0);
    int num = 0;
    if (!colors) {
        num = greedy(a, col.data());
    } else {
        for (int i = 0; i < n; ++i) {
            if (colors[i] < 0 || colors[i] >= n)
                return invalid(std::string(who) + ": row " + std::to_string(i) + ": colour " +
                               std::to_string(colors[i]) + " is outside [0, n)");
            col[i] = colors[i];
            num = std::max(num, col[i] + 1);
        }
        std::vector<int> count((size_t)num, 0);
        for (int i = 0; i < n; ++i)
            ++count[col[i]];
        for (int c = 0; c < num; ++c)
            if (count[c] == 0) {  // the first row past the gap
                int i = 0;
                while (col[i] < c)
                    ++i;
                return invalid(std::string(who) + ": row " + std::to_string(i) + ": colour " + std::to_string(col[i]) +
                               " is in use but colour " + std::to_string(c) + " is not (colours must be 0..C-1)");
            }
        for (int i = 0; i < n; ++i)
            for (int k = a->row_offsets[i]; k < a->row_offsets[i + 1]; ++k) {
                const int j = a->column_indices[k];
                if (j != i && col[j] == col[i])
                    return invalid(std::string(who) + ": row " + std::to_string(i) + " shares colour " +
                                   std::to_string(col[i]) + " with row " + std::to_string(j) + ", which it has an entry in");
            }
    }
    // rows stably sorted by colour: ascending within a colour
    color_off.assign((size_t)num + 1, 0);
    for (int i = 0; i < n; ++i)
        ++color_off[(size_t)col[i] + 1];
    for (int c = 0; c < num; ++c)
        color_off[(size_t)c + 1] += color_off[c];
    perm.assign((size_t)n, 0);
    std::vector<int> inv((size_t)n, 0);
    {
        std::vector<int> pos(color_off.begin(), color_off.end() - 1);
        for (int i = 0; i < n; ++i) {
            inv[i] = pos[col[i]]++;
            perm[inv[i]] = i;
        }
    }
    pro.assign((size_t)n + 1, 0), pci.assign((size_t)std::max(nnz, 1), 0), pva.assign((size_t)std::max(nnz, 1), 0.0);
    permute(a, perm.data(), inv, pro.data(), pci.data(), pva.data());
    return MSPMV_OK;
}

mspmv_status mspmv::ilu0_colored_host(const mspmv_csr_d *a, const int *colors, HostFactor &f)
{
    const char *who = "ilu0_create_colored";
    mspmv_status st = ilu0_check_rows(a, who);
    if (st != MSPMV_OK)
        return st;
    std::vector<int> pro, pci;
    std::vector<double> pva, lu((size_t)std::max(a->num_nonzeros, 1));
    st = color_order(a, colors, who, f.perm, f.color_off, pro, pci, pva);
    if (st != MSPMV_OK)
        return st;
    mspmv_csr_d ap = *a;
    ap.row_offsets = pro.data();
    ap.column_indices = pci.data();
    ap.values = pva.data();
    st = mspmv_ilu0_values(&ap, lu.data());
    if (st != MSPMV_OK) {
        set_error(std::string(mspmv_last_error()) + " [ilu0_create_colored: rows numbered in the colour ordering]");
        return st;
    }
    split_lu(a->num_rows, pro.data(), pci.data(), lu.data(), false, f);
    return MSPMV_OK;
}

// A's structure by mspmv_ic0_nnz's checks (square, consistent offsets, columns in range: all the colouring and the
// permutation need); the rows by mspmv_ic0_factor's own, on the permuted matrix, with its diagonal-shift retries.
mspmv_status mspmv::ic0_colored_host(const mspmv_csr_d *a, const int *colors, HostFactor &f, double *shift)
{
    const char *who = "ic0_create_colored";
    int lnnz = 0;
    mspmv_status st = mspmv_ic0_nnz(a, &lnnz);  // for its checks: L's count is the permuted matrix's, taken below
    if (st != MSPMV_OK)
        return st;
    const int n = a->num_rows;
    std::vector<int> pro, pci;
    std::vector<double> pva;
    st = color_order(a, colors, who, f.perm, f.color_off, pro, pci, pva);
    if (st != MSPMV_OK)
        return st;
    mspmv_csr_d ap = *a;
    ap.row_offsets = pro.data();
    ap.column_indices = pci.data();
    ap.values = pva.data();
    st = mspmv_ic0_nnz(&ap, &lnnz);
    if (st != MSPMV_OK)
        return st;
    f.lro.assign((size_t)n + 1, 0), f.uro.assign((size_t)n + 1, 0);
    f.lci.assign((size_t)std::max(lnnz, 1), 0), f.uci.assign((size_t)std::max(lnnz, 1), 0);
    f.lva.assign((size_t)std::max(lnnz, 1), 0.0), f.uva.assign((size_t)std::max(lnnz, 1), 0.0);
    st = mspmv_ic0_factor(&ap, f.lro.data(), f.lci.data(), f.lva.data(), shift);
    if (st != MSPMV_OK) {
        set_error(std::string(mspmv_last_error()) + " [ic0_create_colored: rows numbered in the colour ordering]");
        return st;
    }
    mspmv_csr_d l = ap;
    l.num_nonzeros = lnnz;
    l.row_offsets = f.lro.data();
    l.column_indices = f.lci.data();
    l.values = f.lva.data();
    st = mspmv_csr_transpose(&l, f.uro.data(), f.uci.data(), f.uva.data());
    f.lci.resize((size_t)lnnz), f.lva.resize((size_t)lnnz), f.uci.resize((size_t)lnnz), f.uva.resize((size_t)lnnz);
    return st;
}
