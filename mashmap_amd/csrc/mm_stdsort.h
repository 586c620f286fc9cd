// mashmap_amd/csrc/mm_stdsort.h -- std::sort of libstdc++ over an array of ids (or of any trivially copied element type T), with the exact
// comparisons and element moves of bits/stl_algo.h (GCC 11 line numbers; the text has not changed since GCC 4.9's move_median_to_first):
//
//   std::__sort                        depth limit 2 * __lg(n), then the final insertion sort        stl_algo.h:1949-1959
//   std::__introsort_loop              partition, recurse into the RIGHT part, loop on the left      :1925-1942
//   std::__unguarded_partition_pivot   __move_median_to_first(first, first + 1, mid, last - 1)       :1900-1907, :79-97
//   std::__unguarded_partition                                                                       :1878-1894
//   std::__partial_sort(f, l, l)       the depth-limit fallback: __heap_select + __sort_heap         :1912-1919, :1642-1650, stl_heap.h
//   std::__final_insertion_sort        __insertion_sort on the first 16, unguarded on the rest       :1861-1872
//   std::__insertion_sort              with its comp(*i, *first) shortcut                            :1819-1837
//   std::__unguarded_linear_insert                                                                   :1799-1813
//   _S_threshold                       16                                                            :1855
//
// Map::mergeMappingsInRange sorts a read's mappings by splitMappingId (computeMap.hpp:1640), a key every member of a chain shares, and
// takes the first member of each run as the chain's representative; filterByGroup and mapSingleQueryFrag sort by keys that tie on tandem
// copies.  Above 16 elements std::sort is introsort, which is not stable: which of several equal elements comes first depends on every
// swap of the partitions.  The reference is built against libstdc++, so the algorithm is restated here move for move;
// tests/hostlogic/stdsort_check.cpp runs it beside std::sort and compares the log of comparator calls and the final permutation.
// For n <= 16 it is __insertion_sort alone.
//
// No recursion: __introsort_loop's call on the right part becomes "push the left part, go on with the right one" on an explicit stack.
// The ranges come up in the order of the original (the right part, with everything below it, before the left), so the comparator is
// called with the same arguments in the same sequence.  Every push happens behind a decrement of the depth limit, so the stack holds at
// most 2 * __lg(n) ranges: 62 for any int n.
// Compiles for the host (g++) and for the device (hipcc).
#pragma once
#include "mm_heap.h"

#define MM_STDSORT_THRESHOLD 16
#define MM_STDSORT_STACK 64

#ifdef MM_STDSORT_COUNT_FALLBACK
static long mm_stdsort_fallbacks = 0;        // test only (stdsort_check.cpp): times the depth limit was reached
#endif

template <class T, class Less>
MM_HD void mm_std_unguarded_linear_insert(T* v, int last, Less less) {
  const T val = v[last];
  int next = last - 1;
  while (less(val, v[next])) { v[last] = v[next]; last = next; next--; }
  v[last] = val;
}

template <class T, class Less>
MM_HD void mm_std_insertion_sort(T* v, int first, int last, Less less) {
  if (first == last) return;
  for (int i = first + 1; i != last; i++) {
    if (less(v[i], v[first])) {
      const T val = v[i];
      for (int j = i; j > first; j--) v[j] = v[j - 1];          // move_backward(first, i, i + 1)
      v[first] = val;
    } else
      mm_std_unguarded_linear_insert(v, i, less);
  }
}

template <class T, class Less>
MM_HD void mm_std_move_median_to_first(T* v, int result, int a, int b, int c, Less less) {
  int pick;
  if (less(v[a], v[b])) {
    if (less(v[b], v[c])) pick = b;
    else if (less(v[a], v[c])) pick = c;
    else pick = a;
  } else if (less(v[a], v[c])) pick = a;
  else if (less(v[b], v[c])) pick = c;
  else pick = b;
  const T t = v[result]; v[result] = v[pick]; v[pick] = t;
}

template <class T, class Less>
MM_HD int mm_std_unguarded_partition(T* v, int first, int last, int pivot, Less less) {
  while (true) {
    while (less(v[first], v[pivot])) first++;
    last--;
    while (less(v[pivot], v[last])) last--;
    if (!(first < last)) return first;
    const T t = v[first]; v[first] = v[last]; v[last] = t;
    first++;
  }
}

// __partial_sort(first, last, last): __heap_select's loop over [middle, last) is empty
template <class T, class Less>
MM_HD void mm_std_heap_sort(T* v, int first, int last, Less less) {
  mm_make_heap(v + first, last - first, less);
  for (int len = last - first; len > 1; len--) mm_pop_heap(v + first, len, less);     // __sort_heap
}

template <class T, class Less>
MM_HD void mm_std_sort(T* v, int n, Less less) {
  if (n <= 0) return;
  if (n > MM_STDSORT_THRESHOLD) {
    int lg = 0;
    while ((n >> (lg + 1)) != 0) lg++;                           // std::__lg
    int sf[MM_STDSORT_STACK], sl[MM_STDSORT_STACK], sd[MM_STDSORT_STACK];
    int top = 0;
    sf[0] = 0; sl[0] = n; sd[0] = 2 * lg; top = 1;
    while (top > 0) {
      top--;
      int first = sf[top], last = sl[top], depth = sd[top];
      while (last - first > MM_STDSORT_THRESHOLD) {
        if (depth == 0) {
#ifdef MM_STDSORT_COUNT_FALLBACK
          mm_stdsort_fallbacks++;
#endif
          mm_std_heap_sort(v, first, last, less);
          break;
        }
        depth--;
        const int mid = first + (last - first) / 2;
        mm_std_move_median_to_first(v, first, first + 1, mid, last - 1, less);
        const int cut = mm_std_unguarded_partition(v, first + 1, last, first, less);
        sf[top] = first; sl[top] = cut; sd[top] = depth; top++;   // the left part waits; the right part is next, as in the original
        first = cut;
      }
    }
    mm_std_insertion_sort(v, 0, MM_STDSORT_THRESHOLD, less);
    for (int i = MM_STDSORT_THRESHOLD; i != n; i++) mm_std_unguarded_linear_insert(v, i, less);   // __unguarded_insertion_sort
  } else
    mm_std_insertion_sort(v, 0, n, less);
}
