// rawdtw_sort_order.h -- the evaluation order of a read's candidates (rmap.cpp:512: std::sort by chaining score, descending), restated once for
// host and device.  std::sort is not stable; where equal scores end up is decided by libstdc++'s introsort, which is deterministic.  This header
// orders a permutation of indexes by score[a] > score[b] and makes exactly that algorithm's comparisons and moves, so that the permutation
// it leaves is the one rawdtw_sort_by_chaining_score (which calls std::sort itself and stays the yardstick) leaves:
//   * the introsort loop, while a range has more than 16 elements: a depth budget of 2 * floor(log2 n); the median of (first + 1, middle, last - 1)
//     goes to the front, an unguarded partition around it, the right part is sorted with the budget that is left, the loop goes on with the left;
//   * a range whose budget ran out is heap-sorted: the heap is made from the last parent down, then popped, each adjust sifting the hole down
//     to a leaf along the better child and pushing the value back up;
//   * one final insertion sort: the first 16 elements guarded (an element that beats the first moves the whole prefix), the rest unguarded.
// No recursion: the right parts wait on an explicit stack.  An entry pushed from a range of budget d has budget d - 1 and every entry above it a
// smaller one, so the stack never holds more than 2 * floor(log2 n) entries; sort_order_desc still checks every push against the capacity it is
// given and returns false (nothing stored past it, the permutation not in order) should one not fit.
#ifndef RAWDTW_SORT_ORDER_H
#define RAWDTW_SORT_ORDER_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAWDTW_SORT_FN __host__ __device__ inline
#else
#define RAWDTW_SORT_FN inline
#endif

namespace rawdtw {
namespace sort_order {

constexpr uint32_t kInsertionMax = 16;   // libstdc++'s _S_threshold: ranges up to here are left to the final insertion sort
constexpr uint32_t kMaxElements = 4096;  // what the stack below is sized for ("chain_max_chains" at its largest)
constexpr uint32_t kStackCap = 2 * 12 + 1; // 2 * floor(log2 kMaxElements) + 1
constexpr uint32_t kRanPartition = 1u, kRanHeap = 2u; // the phases word

struct Range { uint32_t first, last, budget; };

template <typename Score, typename Perm> struct Sorter {
    Score score; // score[i]: readable, indexable
    Perm p;      // the permutation: readable and writable, indexable

    RAWDTW_SORT_FN bool before(const uint32_t a, const uint32_t b) const { return score[a] > score[b]; } // the comparator, on elements
    RAWDTW_SORT_FN void swap(const uint32_t i, const uint32_t j) { const uint32_t t = p[i]; p[i] = p[j]; p[j] = t; }

    // the hole at `hole` of the heap [first, first + len) goes down to a leaf along the child that is not before the other, then `value` is pushed
    // up from there, no higher than `top`
    RAWDTW_SORT_FN void adjust(const uint32_t first, uint32_t hole, const uint32_t len, const uint32_t value)
    {
        const uint32_t top = hole;
        uint32_t child = hole;
        while (child < (len - 1) / 2) {
            child = 2 * (child + 1);
            if (before(p[first + child], p[first + child - 1])) child--;
            p[first + hole] = p[first + child];
            hole = child;
        }
        if ((len & 1u) == 0 && child == (len - 2) / 2) { // an even heap's last parent has one child
            child = 2 * (child + 1);
            p[first + hole] = p[first + child - 1];
            hole = child - 1;
        }
        while (hole > top) {
            const uint32_t parent = (hole - 1) / 2;
            if (!before(p[first + parent], value)) break;
            p[first + hole] = p[first + parent];
            hole = parent;
        }
        p[first + hole] = value;
    }
    RAWDTW_SORT_FN void heap_sort(const uint32_t first, uint32_t last)
    {
        const uint32_t len = last - first;
        if (len >= 2)
            for (uint32_t parent = (len - 2) / 2;; parent--) {
                adjust(first, parent, len, p[first + parent]);
                if (parent == 0) break;
            }
        while (last - first > 1) {
            last--;
            const uint32_t value = p[last];
            p[last] = p[first];
            adjust(first, 0, last - first, value);
        }
    }
    // the median of a, b, c (positions) to `dst`
    RAWDTW_SORT_FN void median_to(const uint32_t dst, const uint32_t a, const uint32_t b, const uint32_t c)
    {
        if (before(p[a], p[b])) {
            if (before(p[b], p[c])) swap(dst, b);
            else if (before(p[a], p[c])) swap(dst, c);
            else swap(dst, a);
        } else if (before(p[a], p[c])) swap(dst, a);
        else if (before(p[b], p[c])) swap(dst, c);
        else swap(dst, b);
    }
    // [first, last), more than 16 elements: the pivot to `first`, the rest parted around it; the cut.  Unguarded in the library: the median has
    // an element on either side that stops each scan inside the range.  The range checks here never decide anything for scores that order
    // (they would for a NaN, where std::sort itself is undefined): they keep every index inside [first, last) whatever the scores are.
    RAWDTW_SORT_FN uint32_t partition(const uint32_t first, const uint32_t last)
    {
        median_to(first, first + 1, first + (last - first) / 2, last - 1);
        const uint32_t pivot = p[first];
        uint32_t lo = first + 1, hi = last;
        for (;;) {
            while (lo < last - 1 && before(p[lo], pivot)) lo++;
            if (hi > first + 1) hi--;
            while (hi > first + 1 && before(pivot, p[hi])) hi--;
            if (!(lo < hi)) return lo;
            swap(lo, hi);
            lo++;
        }
    }
    RAWDTW_SORT_FN void insert_unguarded(uint32_t at)
    {
        const uint32_t value = p[at];
        while (at > 0 && before(value, p[at - 1])) { p[at] = p[at - 1]; at--; } // (at > 0: as above -- the library leaves it out where an earlier element is known to stop the scan)
        p[at] = value;
    }
    RAWDTW_SORT_FN void insertion_sort(const uint32_t n)
    {
        const uint32_t guarded = n < kInsertionMax ? n : kInsertionMax;
        for (uint32_t i = 1; i < guarded; i++) {
            if (before(p[i], p[0])) { // before everything so far: the prefix moves up as a whole
                const uint32_t value = p[i];
                for (uint32_t j = i; j > 0; j--) p[j] = p[j - 1];
                p[0] = value;
            } else insert_unguarded(i);
        }
        for (uint32_t i = guarded; i < n; i++) insert_unguarded(i);
    }
    RAWDTW_SORT_FN bool run(const uint32_t n, Range *stack, const uint32_t stack_cap, uint32_t *phases)
    {
        uint32_t ran = 0;
        bool ok = true;
        if (n > kInsertionMax) {
            uint32_t lg = 0;
            while ((n >> (lg + 1)) != 0) lg++;
            uint32_t sp = 0, first = 0, last = n, budget = 2 * lg;
            for (;;) {
                while (last - first > kInsertionMax) {
                    if (budget == 0) { heap_sort(first, last); ran |= kRanHeap; break; }
                    budget--;
                    const uint32_t cut = partition(first, last);
                    ran |= kRanPartition;
                    if (last - cut > kInsertionMax) { // (a right part of at most 16 would only be looked at and left)
                        if (sp >= stack_cap) { ok = false; break; }
                        stack[sp++] = Range{cut, last, budget};
                    }
                    last = cut;
                }
                if (!ok || sp == 0) break;
                sp--;
                first = stack[sp].first; last = stack[sp].last; budget = stack[sp].budget;
            }
        }
        if (ok) insertion_sort(n);
        if (phases) *phases = ran;
        return ok;
    }
};

// perm[0 .. n) -- any permutation of 0 .. n-1 on entry, the identity for std::sort's result on the scores as given -- ordered by score, descending,
// with std::sort's decisions.  phases: kRanPartition | kRanHeap.  false: the stack was too small (never with kStackCap for n <= kMaxElements).
template <typename Score, typename Perm>
RAWDTW_SORT_FN bool sort_order_desc(Score score, Perm perm, const uint32_t n, Range *stack, const uint32_t stack_cap, uint32_t *phases)
{
    Sorter<Score, Perm> s{score, perm};
    return s.run(n, stack, stack_cap, phases);
}

} // namespace sort_order
} // namespace rawdtw

#endif
