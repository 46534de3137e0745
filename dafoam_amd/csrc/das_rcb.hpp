// Recursive coordinate bisection of a set of points (host only, no HIP).  The points are the entries of an index array;
// centre(index, axis) gives their coordinates.  One rule for every caller: a range is cut across its widest axis (the lowest
// axis wins a tie of extents) in the order (coordinate, index) - a total order, so the set on each side of a cut is determined
// whatever nth_element does inside a half - and the lower half is processed first.
#pragma once
#include <algorithm>
#include <vector>

namespace das {

// idx[b, mid) precede idx[mid, e) in the order (coordinate on the widest axis of idx[b, e), index)
template <class Centre>
inline void rcb_cut(std::vector<int>& idx, const Centre& centre, long long b, long long mid, long long e) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (long long q = b; q < e; q++)
        for (int d = 0; d < 3; d++) { const double x = centre(idx[q], d); lo[d] = std::min(lo[d], x); hi[d] = std::max(hi[d], x); }
    int ax = 0;
    for (int d = 1; d < 3; d++) if (hi[d] - lo[d] > hi[ax] - lo[ax]) ax = d;
    std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e, [&](int a, int b2) {
        const double xa = centre(a, ax), xb = centre(b2, ax);
        return xa < xb || (xa == xb && a < b2);
    });
}

// K parts of (almost) equal size: a range that is to hold na parts gives nl = na / 2 of them, and that share of its entries, to
// the lower side.  partOf[index] = part of every entry of idx (the other entries of partOf are left alone); idx ends grouped by part.
template <class Centre>
inline void rcb_parts(std::vector<int>& idx, const Centre& centre, int K, std::vector<int>& partOf) {
    struct Rg { long long b, e; int a0, na; };
    std::vector<Rg> stack{{0, (long long)idx.size(), 0, K}};
    while (!stack.empty()) {
        const Rg r = stack.back();
        stack.pop_back();
        if (r.na == 1) { for (long long q = r.b; q < r.e; q++) partOf[idx[q]] = r.a0; continue; }
        const int nl = r.na / 2;
        const long long mid = r.b + (r.e - r.b) * nl / r.na;
        rcb_cut(idx, centre, r.b, mid, r.e);
        stack.push_back({mid, r.e, r.a0 + nl, r.na - nl});
        stack.push_back({r.b, mid, r.a0, nl});
    }
}

// Halving at (b + e) / 2 until a range holds at most maxLeaf entries.  idx ends grouped by leaf, leaf l = idx[leafOff[l],
// leafOff[l + 1]): the leaves are numbered by ascending start.
template <class Centre>
inline void rcb_leaves(std::vector<int>& idx, const Centre& centre, long long maxLeaf, std::vector<long long>& leafOff) {
    struct Rg { long long b, e; };
    std::vector<Rg> stack{{0, (long long)idx.size()}};
    leafOff.clear();
    while (!stack.empty()) {
        const Rg r = stack.back();
        stack.pop_back();
        if (r.e - r.b <= maxLeaf) { leafOff.push_back(r.b); continue; }  // (lower half first: the starts come out ascending)
        const long long mid = (r.b + r.e) / 2;
        rcb_cut(idx, centre, r.b, mid, r.e);
        stack.push_back({mid, r.e});
        stack.push_back({r.b, mid});
    }
    leafOff.push_back((long long)idx.size());
}

}  // namespace das
