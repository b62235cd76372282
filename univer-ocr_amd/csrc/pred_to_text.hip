// PredToText: the device form of the reference's last stage (interpreter/interpreter.py:574-614 PredToText._func1).  Per
// line, pred is the Char net's raw output (W, n_chars), one row per column window:
//   maximum     of every row (:597); a row whose maximum == 0.0 (-0.0 included) contributes nothing (:598), a row that
//               holds a NaN neither (np.max is NaN there and nothing equals NaN)
//   candidates  every column that EQUALS its row's maximum (:600-601), ordered by row and inside a row by column (:602)
//   walk        prev = none; id 0 (the tab) resets prev and emits nothing; an id similar to prev is skipped and leaves
//               prev alone; every other id is emitted and becomes prev (:603-613).  similar(a, b) = a in the pair of b
//               (primitives/__init__.py:16-54): `cls` gives every id the index of its pair, -1 for an unpaired one.
// After any id that is not the tab, prev lies in that id's pair class (it was kept BECAUSE it was similar, or it became
// the id), so the walk needs no state: candidate s[i] is emitted iff s[i] != 0 and not (cls[s[i]] >= 0 and i > 0 and
// s[i-1] != 0 and cls[s[i-1]] == cls[s[i]]).  "i - 1" is the previous CANDIDATE: rows without candidates are passed over.
//
// All lines of a call travel together, PT_LINES per launch pair, their pointers, sizes and the class table in a by-value
// kernel argument (no device allocation, no copy, no host synchronisation: asynchronous and capturable).  A block takes
// PT_ROWS consecutive rows of one line.  Launches per PT_LINES lines:
//   1. pred_to_text_scan  a wave takes a row: 16-byte loads between a scalar head and tail, the values parked in LDS by
//                         column; maximum and NaN flag by a wave reduction; ballots of value == maximum give the row's
//                         256-bit candidate mask.  The block then decides its emissions as if nothing came before it
//                         and leaves in the ctx workspace: the masks (32 bytes per row) and its summary {first
//                         candidate, last candidate, emissions}
//   2. pred_to_text_emit  the same blocks: from the summaries of the blocks of ITS line in front of it a block gets the
//                         candidate before its first one and the number of ids emitted before it (a block in front
//                         emits one less than its summary says exactly when its first candidate is suppressed by ITS
//                         predecessor), decides its emissions from the masks (a prefix sum over the rows' candidates
//                         is a popcount of mask words), compacts them by a second prefix sum and writes ids[pos] for
//                         pos < cap; the last block of a line writes count
// pred crosses HBM once.  Comparisons only, no floating-point arithmetic (binary16 is widened to float32, which is
// exact): results EQUAL the reference's in every dtype.  No atomics: bit-identical run to run.
#include "entry_batch.h"

namespace {

constexpr int PT_NT = 256;               // threads per block of both kernels
constexpr int PT_WAVES = PT_NT / 64;
constexpr int PT_ROWS = 64;              // rows of a line per block
constexpr int PT_LINES = 64;             // lines per launch pair (the descriptor is a kernel argument: 4 KB at most)
constexpr int PT_MAX_CHARS = 256;        // ids are bytes; a row's candidate mask is PT_WORDS 64-bit words
constexpr int PT_WORDS = PT_MAX_CHARS / 64;

struct PTLine {
    const void* pred;
    unsigned char* ids;
    int* count;
    int w, cap;
};
struct PTBatch {
    PTLine line[PT_LINES];
    int block_first[PT_LINES + 1];       // first block of line i in the grid (both kernels)
    short cls[PT_MAX_CHARS];             // pair index of every id, -1: unpaired
    int n, n_chars;
};
static_assert(sizeof(PTBatch) <= 4096, "the descriptor travels as a kernel argument");

struct PTSummary {                       // of one block, as if no candidate came before it
    int first, last;                     // its first and last candidate, -1: it has none
    int emitted;
    int pad;
};

struct PTShared {
    unsigned long long cand[PT_ROWS][PT_WORDS];   // candidate masks: bit (c & 63) of word c >> 6 = column c
    unsigned long long emit[PT_ROWS][PT_WORDS];   // the candidates that are emitted
    int row_prev[PT_ROWS];               // the candidate before the row's first one, 0: none (a tab suppresses nothing either)
    int row_count[PT_ROWS], row_first[PT_ROWS + 1];   // emissions of a row, and of the rows before it in the block
    short cls[PT_MAX_CHARS];
    int first, last;
};

__device__ __forceinline__ int pt_highest(unsigned long long word) { return 63 - __clzll((long long)word); }

// s[i] = cur is emitted after s[i - 1] = prev (0: no candidate before it, or the tab)
__device__ __forceinline__ bool pt_emitted(const short* cls, int cur, int prev) {
    return cur != 0 && !(cls[cur] >= 0 && prev != 0 && cls[prev] == cls[cur]);
}

// The emissions of the block whose candidate masks are in s.cand (rows past the line's end: zero), prev_in the candidate
// in front of the block (0: none).  Fills s.emit, s.row_count, s.row_first[0 .. PT_ROWS], s.first, s.last.  Every thread
// of the block calls this (it contains barriers); s.cand and s.cls are complete before the call.
__device__ __forceinline__ void pt_block_emissions(PTShared& s, int prev_in) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
    if (tid == 0) {                                                  // the candidate in front of every row
        int prev = prev_in, first = -1, last = -1;
        for (int r = 0; r < PT_ROWS; ++r) {
            s.row_prev[r] = prev;
            for (int k = 0; k < PT_WORDS; ++k)
                if (s.cand[r][k]) {
                    prev = last = 64 * k + pt_highest(s.cand[r][k]);
                    if (first < 0) first = 64 * k + __ffsll((long long)s.cand[r][k]) - 1;
                }
        }
        s.first = first, s.last = last;
    }
    __syncthreads();
    for (int r = wave; r < PT_ROWS; r += PT_WAVES) {
        int before = s.row_prev[r], count = 0;                       // `before`: the last candidate in front of word k
        for (int k = 0; k < PT_WORDS; ++k) {
            const unsigned long long word = s.cand[r][k], below = word & ((1ull << lane) - 1ull);
            const int cur = 64 * k + lane, prev = below ? 64 * k + pt_highest(below) : before;
            const unsigned long long e = __ballot((int)((word >> lane) & 1ull) && pt_emitted(s.cls, cur, prev));
            if (lane == 0) s.emit[r][k] = e;
            count += __popcll(e);
            if (word) before = 64 * k + pt_highest(word);
        }
        if (lane == 0) s.row_count[r] = count;
    }
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int r = 0; r < PT_ROWS; ++r) s.row_first[r] = sum, sum += s.row_count[r];
        s.row_first[PT_ROWS] = sum;
    }
    __syncthreads();
}

__device__ __forceinline__ void pt_load_cls(PTShared& s, const PTBatch& b) {
    for (int i = threadIdx.x; i < PT_MAX_CHARS; i += PT_NT) s.cls[i] = i < b.n_chars ? b.cls[i] : (short)-1;
}

// ---- 1. candidate masks of every row, summary of every block --------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PT_NT) void pred_to_text_scan(const PTBatch b, unsigned long long* __restrict__ masks,
                                                           PTSummary* __restrict__ summary) {
    using CT = std::conditional_t<std::is_same_v<T, double>, double, float>;   // binary16 -> float32 is exact
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    __shared__ PTShared s;
    __shared__ CT vals[PT_WAVES][PT_MAX_CHARS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int line = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const int row0 = (blockIdx.x - b.block_first[line]) * PT_ROWS;
    const int w = b.line[line].w, n_chars = b.n_chars;
    const int nrows = w - row0 < PT_ROWS ? w - row0 : PT_ROWS;
    pt_load_cls(s, b);
    for (int r = wave; r < PT_ROWS; r += PT_WAVES) {                  // (a wave reads only what it parked itself)
        unsigned long long word[PT_WORDS] = {};
        if (r < nrows) {
            const T* p = (const T*)b.line[line].pred + (size_t)(row0 + r) * n_chars;
            const auto [head, nvec, tail] = eb_split(p, n_chars);
            CT mx = -INFINITY;
            bool nan = false;
            const auto take = [&](int col, CT v) {
                vals[wave][col] = v;
                nan |= v != v;
                mx = v > mx ? v : mx;
            };
            if (lane < head) take(lane, (CT)p[lane]);
            const V* pv = reinterpret_cast<const V*>(p + head);
            for (int i = lane; i < nvec; i += 64) {
                const V v = pv[i];
#pragma unroll
                for (int j = 0; j < VEC; ++j) take(head + i * VEC + j, (CT)v[j]);
            }
            if (lane < tail) take(head + nvec * VEC + lane, (CT)p[head + nvec * VEC + lane]);
            mx = __shfl(wave_reduce_max(mx), 0, 64);
            const bool live = __ballot(nan) == 0ull && mx != (CT)0;   // (-0.0 == 0.0: such a row contributes nothing)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int k = 0; k < PT_WORDS; ++k) {
                const int col = 64 * k + lane;
                const CT v = vals[wave][col < n_chars ? col : 0];
                word[k] = __ballot(live && col < n_chars && v == mx);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next row's values wait for these reads
            __builtin_amdgcn_wave_barrier();
        }
        if (lane < PT_WORDS) {
            unsigned long long mine = word[0];
#pragma unroll
            for (int k = 1; k < PT_WORDS; ++k) mine = lane == k ? word[k] : mine;
            s.cand[r][lane] = mine;
            if (r < nrows) masks[((size_t)blockIdx.x * PT_ROWS + r) * PT_WORDS + lane] = mine;
        }
    }
    pt_block_emissions(s, 0);
    if (tid == 0) summary[blockIdx.x] = PTSummary{s.first, s.last, s.row_first[PT_ROWS], 0};
}

// ---- 2. emissions of every block, compacted -------------------------------------------------------------------------
__global__ __launch_bounds__(PT_NT) void pred_to_text_emit(const PTBatch b, const unsigned long long* __restrict__ masks,
                                                           const PTSummary* __restrict__ summary) {
    __shared__ PTShared s;
    __shared__ int s_prev, s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int line = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const int first_block = b.block_first[line], last_block = b.block_first[line + 1] - 1;
    const int row0 = (blockIdx.x - first_block) * PT_ROWS;
    const int w = b.line[line].w, cap = b.line[line].cap;
    const int nrows = w - row0 < PT_ROWS ? w - row0 : PT_ROWS;
    pt_load_cls(s, b);
    for (int i = tid; i < PT_ROWS * PT_WORDS; i += PT_NT)
        s.cand[i / PT_WORDS][i % PT_WORDS] = i / PT_WORDS < nrows ? masks[(size_t)blockIdx.x * PT_ROWS * PT_WORDS + i] : 0ull;
    __syncthreads();
    if (tid == 0) {                                                  // the blocks of this line in front of this one, in order
        int prev = 0, base = 0;
        for (int j = first_block; j < (int)blockIdx.x; ++j) {
            const PTSummary o = summary[j];
            if (o.first >= 0) {
                base += o.emitted - (pt_emitted(s.cls, o.first, 0) && !pt_emitted(s.cls, o.first, prev) ? 1 : 0);
                prev = o.last;
            }
        }
        s_prev = prev, s_base = base;
    }
    __syncthreads();
    pt_block_emissions(s, s_prev);
    unsigned char* ids = b.line[line].ids;
    for (int r = wave; r < nrows; r += PT_WAVES) {
        int pos = s_base + s.row_first[r];
        for (int k = 0; k < PT_WORDS; ++k) {
            const unsigned long long e = s.emit[r][k];
            if ((e >> lane) & 1ull) {
                const int at = pos + __popcll(e & ((1ull << lane) - 1ull));
                if (at < cap) ids[at] = (unsigned char)(64 * k + lane);
            }
            pos += __popcll(e);
        }
    }
    if (tid == 0 && (int)blockIdx.x == last_block) *b.line[line].count = s_base + s.row_first[PT_ROWS];
}

}  // namespace

extern "C" {

int uocr_pred_to_text(uocr_ctx* ctx, int dtype, int n_lines, const void* const* pred, const int* w, int n_chars,
                      const int* cls, unsigned char* const* ids, const int* cap, int* const* count) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_lines >= 0);
    if (n_lines == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, pred && w && cls && ids && cap && count);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    UOCR_REQUIRE(ctx, n_chars >= 1 && n_chars <= PT_MAX_CHARS);
    for (int k = 0; k < n_chars; ++k) UOCR_REQUIRE(ctx, cls[k] >= -1 && cls[k] < n_chars);
    const auto blocks = [&](int i) { return ((long long)w[i] + PT_ROWS - 1) / PT_ROWS; };
    // everything is checked before the first launch: an error leaves every output as it was
    long long max_blocks = 0;
    for (int first = 0; first < n_lines; first += PT_LINES) {
        const int group = eb_group_size(n_lines, first, PT_LINES);
        for (int i = first; i < first + group; ++i) {
            UOCR_REQUIRE(ctx, w[i] >= 1 && cap[i] >= 0);
            UOCR_REQUIRE(ctx, pred[i] && count[i] && (ids[i] || cap[i] == 0));
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(pred[i]) % elem == 0);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(count[i]) % sizeof(int) == 0);
        }
        const long long total = eb_group_blocks(first, group, blocks);
        if (total < 0) UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "lines %d..: too many blocks for one grid", first);
        max_blocks = total > max_blocks ? total : max_blocks;
    }
    // workspace: the masks of every row and the summary of every block of one launch pair; the pairs of a call follow
    // each other on the stream
    const size_t mask_bytes = (size_t)max_blocks * PT_ROWS * PT_WORDS * sizeof(unsigned long long);
    if (int rc = uocr_need_workspace(ctx, mask_bytes + (size_t)max_blocks * sizeof(PTSummary))) return rc;
    unsigned long long* masks = (unsigned long long*)ctx->workspace;
    PTSummary* summary = (PTSummary*)((char*)ctx->workspace + mask_bytes);
    int launches = 0;
    for (int first = 0; first < n_lines; first += PT_LINES) {
        PTBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_lines, first, PT_LINES);
        eb_block_first(first, b.n, b.block_first, blocks);
        b.n_chars = n_chars;
        for (int k = 0; k < n_chars; ++k) b.cls[k] = (short)cls[k];
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            b.line[i].pred = pred[s], b.line[i].ids = ids[s], b.line[i].count = count[s];
            b.line[i].w = w[s], b.line[i].cap = cap[s];
        }
        const dim3 grid((unsigned)b.block_first[b.n]);
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL(pred_to_text_scan<T>, grid, dim3(PT_NT), 0, ctx->stream, b, masks, summary);
            UOCR_LAUNCH_CHECK(ctx);
        });
        hipLaunchKernelGGL(pred_to_text_emit, grid, dim3(PT_NT), 0, ctx->stream, b, (const unsigned long long*)masks,
                           (const PTSummary*)summary);
        UOCR_LAUNCH_CHECK(ctx);
        launches += 2;
    }
    uocr_note(ctx, UOCR_REPORT_PRED_TO_TEXT, PT_ROWS, PT_LINES, launches);
    return UOCR_OK;
}

int uocr_ctx_last_pred_to_text(uocr_ctx* ctx, int* rows_per_block, int* lines_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_PRED_TO_TEXT, rows_per_block, lines_per_launch, launches);
}

}  // extern "C"
