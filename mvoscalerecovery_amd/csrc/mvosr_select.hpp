// mvosr_select.hpp — exact order statistics of a list of 64-bit keys by radix select, one wavefront per list.  Shared by
// mvosr_statictri.hip (np.median of the inverse heights, read from global memory) and mvosr_featdist.hip (np.median of a
// population's y, read from LDS).  The text was moved here from mvosr_statictri.hip; what differs between the users — where the
// list lives and how a value becomes a key — is the caller's `for_each`.
//
// for_each(visit) calls visit(counted, key) once per entry, 64 entries a step, EVERY lane of the wave in every step (the visitors
// hold ballots); a lane past the end, or an entry that is not part of the list, passes counted == false.  Keys order like the
// values they stand for (the patterns of non-negative doubles do; see fd_key in mvosr_featdist.hip for signed ones).
#pragma once

#include "mvosr_device.hpp"

namespace mvosr {

// The key of rank `rank` (0-based, ascending) among the counted entries: four bits a pass from the top; lane b < 16 counts the
// entries whose key continues the prefix with digit b.  Each pass visits the list once.
template <class ForEach>
__device__ __forceinline__ unsigned long long wave_radix_select(ForEach for_each, int rank) {
    const int lane = lane_id();
    unsigned long long prefix = 0ull;
    for (int shift = 60; shift >= 0; shift -= 4) {
        int mine = 0;
        for_each([&](bool counted, unsigned long long p) {
            const bool match = counted && (shift == 60 || (p >> (shift + 4)) == (prefix >> (shift + 4)));
            const int digit = match ? (int)((p >> shift) & 15ull) : -1;
            if (__ballot(match) == 0ull) return;
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                const int c = __popcll(__ballot(digit == b));
                mine += lane == b ? c : 0;
            }
        });
        const int incl = wave_scan_incl(lane < 16 ? mine : 0);
        // (the rank lies inside the entries that share the prefix, so a lane below 16 answers)
        const int sel = max(__ffsll((long long)__ballot(lane < 16 && incl > rank)) - 1, 0);
        const int before = __shfl(incl, max(sel - 1, 0));
        rank -= sel > 0 ? before : 0;
        prefix |= (unsigned long long)sel << shift;
    }
    return prefix;
}

// The middle of n >= 1 counted entries as np.median takes it: lo = the key of rank (n - 1) / 2 and, for an even n, hi = the key of
// rank n / 2 — lo again where it occurs often enough, else the smallest key above it (one more visit of the list).  Odd n: hi = lo.
template <class ForEach>
__device__ __forceinline__ void wave_middle_keys(ForEach for_each, int n, unsigned long long &lo, unsigned long long &hi) {
    lo = wave_radix_select(for_each, (n - 1) >> 1);
    hi = lo;
    if (n & 1) return;
    int le = 0;
    unsigned long long above = ~0ull;
    const unsigned long long vlo = lo;
    for_each([&](bool counted, unsigned long long p) {
        le += (counted && p <= vlo) ? 1 : 0;
        above = (counted && p > vlo && p < above) ? p : above;
    });
    le = wave_sum(le);
    above = wave_min_u64(above);
    hi = le > (n >> 1) ? lo : above;
}

}  // namespace mvosr
