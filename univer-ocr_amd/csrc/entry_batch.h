// What the batched page stages (line_crop.hip, char_label.hip, rotate.hip, pred_to_text.hip, pack_lines.hip) share.  The entries of a call travel in by-value
// kernel arguments, a GROUP of at most `entries` per launch, next to the prefix sum of their block counts; a block finds
// its entry by a binary search in it; contiguous ranges move as 16-byte accesses between a scalar head and tail.  The
// descriptor structs stay with their kernels.  A launcher writes the block count of an entry ONCE, as a function `blocks`
// of the entry's index in the call: eb_group_blocks takes it when a group is checked, eb_block_first when its descriptor
// is filled.  No floating-point arithmetic in here: no includer needs special flags.
#pragma once
#include "uocr_common.h"

template <typename T>
struct EBVec {                      // 16 bytes of T
    static constexpr int N = 16 / sizeof(T);
    using type = T __attribute__((ext_vector_type(16 / sizeof(T))));
};

// the entry whose blocks [first[i], first[i + 1]) contain block b (block-uniform; entries without blocks are passed over)
__device__ __forceinline__ int eb_entry_of(const int* first, int n, int b) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// n elements from p on: `head` elements up to a 16-byte border, `nvec` vectors of EBVec<T>::N, `tail` elements
struct EBSplit { int head, nvec, tail; };
template <typename T>
__device__ __forceinline__ EBSplit eb_split(const T* p, int n) {
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
    head = head < n ? head : n;
    const int nvec = (n - head) / EBVec<T>::N;
    return {head, nvec, n - head - nvec * EBVec<T>::N};
}

// bytes per element of a storage dtype; 0, and the message, for any other: `if (!elem) return UOCR_ERR_DTYPE;`
inline size_t eb_storage_elem(uocr_ctx* ctx, int dtype) {
    const int base = UOCR_DTYPE_BASE(dtype);
    if (base != UOCR_F32 && base != UOCR_F64 && base != UOCR_F16) UOCR_FAIL(ctx, 0, "unknown dtype %d", dtype);
    return base == UOCR_F64 ? 8 : base == UOCR_F32 ? 4 : 2;
}

// entries in the group that starts at entry `first` of n
inline int eb_group_size(int n, int first, int entries) { return n - first < entries ? n - first : entries; }

// blocks of the group of `count` entries from entry `first` on (blocks(i) >= 0 each), or -1: too many for one grid
template <typename Blocks>
inline long long eb_group_blocks(int first, int count, Blocks blocks) {
    long long sum = 0;
    for (int i = first; i < first + count; ++i) sum += blocks(i);
    return sum <= INT32_MAX ? sum : -1;
}

// block_first[0 .. count] of a group that fits one grid: the first block of every entry, then the size of the grid
template <typename Blocks>
inline void eb_block_first(int first, int count, int* block_first, Blocks blocks) {
    block_first[0] = 0;
    for (int i = 0; i < count; ++i) block_first[i + 1] = block_first[i] + (int)blocks(first + i);
}
