// sbox_bounds_check.cpp -- TEST ARTEFACT.  csrc/sbox_bounds.h compiled for the host behind a flat extern "C" face, so that
// tests/test_sbox_bounds_hostcore.py can check the helper every signed box backward kernel calls without a GPU.  Nothing in
// the product links or loads this file.
#include "../../diffqcqp_amd/csrc/sbox_bounds.h"

extern "C" __attribute__((visibility("default"))) void sbox_bounds_many(long n, const double* lo, const double* hi,
                                                                        const double* v, double* lo_eff, double* hi_eff,
                                                                        int* keep_lo, int* keep_hi)
{
    for (long i = 0; i < n; ++i) {
        const dqq::SBoxBounds b = dqq::sbox_bounds(lo[i], hi[i], v[i]);
        lo_eff[i] = b.lo;
        hi_eff[i] = b.hi;
        keep_lo[i] = b.keep_lo ? 1 : 0;
        keep_hi[i] = b.keep_hi ? 1 : 0;
    }
}
