// rtm_grade_index.h — the index arithmetic of rtm_grade's 3D LUT (include/rtm.h: rtm_grade, step 6), in one function that the
// kernel (rtm_grade_kernel.h) and host code compile alike: lut_selftest.cpp checks it on the CPU, under the sanitizers, on
// the values where a lattice index can go wrong.  No HIP header is needed to include this file.
#ifndef RTM_GRADE_INDEX_H
#define RTM_GRADE_INDEX_H

#if defined(__HIP__) || defined(__CUDACC__)
#define RTM_GRADE_HD __host__ __device__
#else
#define RTM_GRADE_HD
#endif

namespace rtm {

// s: a channel's lattice coordinate (y - lo) inv, ANY float; n: the table's size per axis, 2..256.
// The cell i in [0, n - 2] and the fraction f in [0, 1] inside it, so that i and i + 1 are lattice indices for every s:
//   s = (s > 0) ? min(s, n - 1) : 0   a NaN, a negative number and -0 give +0; +inf and anything past the last point n - 1
//   i = min((int)s, n - 2)            (s is in [0, 255] here: the conversion is defined)
//   f = s - i                         exact: s and i are within a factor of two, or i = 0; s = n - 1 gives i = n - 2, f = 1
RTM_GRADE_HD inline void gr_lut_index(float s, const int n, int& i, float& f) {
    const float last = (float)(n - 1);
    s = (s > 0.0f) ? (s < last ? s : last) : 0.0f;
    const int c = (int)s;
    i = c < n - 2 ? c : n - 2;
    f = s - (float)i;
}

}  // namespace rtm
#endif
