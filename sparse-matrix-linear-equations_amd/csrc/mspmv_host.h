// mspmv_host.h -- what the host-only translation units (mspmv_ic0.cpp, mspmv_ilu0.cpp, mspmv_color.cpp,
// mspmv_spai.cpp, mspmv_cache.cpp, mspmv_streams.cpp) share with each other and with the HIP ones (mspmv_internal.h includes it).  Needs no HIP.
// Not installed; the public boundary is include/mspmv.h.
#pragma once

#include <string>
#include <vector>

#include "mspmv.h"

namespace mspmv {

void set_error(const std::string &msg);  // the thread's mspmv_last_error text (mspmv_api.hip)

inline mspmv_status invalid(const std::string &msg)
{
    set_error(msg);
    return MSPMV_ERR_INVALID;
}

// Slots of a device's stream pool (mspmv_streams.cpp keeps who holds which, mspmv_api.hip the streams): the
// hardware queues a process opens by default, so that streams created back to back, one per slot, land each on
// a queue of its own.  More streams than queues would only share them again.
constexpr int kStreamPool = 4;

// The structure of a host CSR: arrays present, row_offsets[0] == 0, offsets monotone and ending in num_nonzeros,
// columns in [0, num_cols).  Else MSPMV_ERR_INVALID, the message prefixed with "who: ".  Squareness is the
// caller's to ask for, in its own words.
inline mspmv_status check_csr(const mspmv_csr_d *a, const char *who)
{
    const std::string w = std::string(who) + ": ";
    if (!a || a->num_rows < 0 || a->num_cols < 0 || a->num_nonzeros < 0 || !a->row_offsets ||
        (a->num_nonzeros > 0 && (!a->column_indices || !a->values)))
        return invalid(w + "bad arguments");
    const int m = a->num_rows;
    for (int r = 0; r < m; ++r)
        if (a->row_offsets[r + 1] < a->row_offsets[r])
            return invalid(w + "row_offsets not monotone");
    if (a->row_offsets[0] != 0 || a->row_offsets[m] != a->num_nonzeros)
        return invalid(w + "row_offsets inconsistent with num_nonzeros");
    for (int k = 0; k < a->num_nonzeros; ++k)
        if (a->column_indices[k] < 0 || a->column_indices[k] >= a->num_cols)
            return invalid(w + "column index out of range");
    return MSPMV_OK;
}

// Square, consistent CSR whose rows ascend strictly and hold their diagonal (mspmv_ilu0.cpp); else
// MSPMV_ERR_INVALID, the message (prefixed with who) naming the first offending row.
mspmv_status ilu0_check_rows(const mspmv_csr_d *a, const char *who);

// A factor's two triangles on the host, as the device upload takes them (mspmv_tri.hip): L and U (IC(0): L^T,
// diagonal first), and for a multi-colour factor the ordering -- row i of the permuted matrix is row perm[i] of
// A, colour c's rows are [color_off[c], color_off[c + 1]).  perm and color_off stay empty for a natural-order one.
struct HostFactor {
    std::vector<int> perm, color_off;
    std::vector<int> lro, lci, uro, uci;
    std::vector<double> lva, uva;
};

// An LU pattern (rows ascending, diagonal present) split into f's L -- the strictly lower entries, then a stored
// 1.0 diagonal when unit_diag (k_trsv_tagged divides by it: exactly) -- and U, diagonal first (mspmv_ilu0.cpp).
void split_lu(int n, const int *ro, const int *ci, const double *va, bool unit_diag, HostFactor &f);

// The host side of mspmv_ilu0_create_colored (mspmv_color.cpp): the checks, the ordering and the factor of the
// permuted matrix, split into L (strictly lower) and U (diagonal first).
mspmv_status ilu0_colored_host(const mspmv_csr_d *a, const int *colors, HostFactor &f);
// The host side of mspmv_ic0_create_colored: the same colour checks and ordering, then mspmv_ic0_factor of the
// permuted matrix (L, diagonal last) and its mspmv_csr_transpose (diagonal first); *shift (nullable): the shift used.
mspmv_status ic0_colored_host(const mspmv_csr_d *a, const int *colors, HostFactor &f, double *shift);

}  // namespace mspmv
