// Training pages made on the device: the reference's generate_data (image_generator/generate.py: LayeredImage.add_paragraph)
// as two calls, both integer arithmetic only (tests/page_rules.py restates every rule in NumPy).
//   uocr_page_layout  random texts in random faces, wrapped, measured with the atlas metrics and placed: per page the int32
//                     tables paragraphs (x0, y0, w, h, face, n_lines, first_line, attempt), lines (left, y_ascent, width,
//                     first_glyph, n_glyphs), glyphs (pen, id) and counts (paragraphs, lines, glyphs, 0)
//   uocr_page_render  a gather over the tables: every pixel finds its paragraph, line and glyph and writes its 14 label
//                     values -- image, monochrome, paragraph, line (2), char (9)
// Random numbers are counter based: draw `slot` of attempt `attempt` of page `page` is splitmix64 of
// seed + (((page * 32 + attempt) * 1024 + slot) + 1) * 0x9E3779B97F4A7C15, scaled to [lo, hi] by a 32 x 32 bit product.  Any
// lane computes any draw, so nothing is handed from lane to lane but maxima and ballots.
//
// Layout: a block per page.  Its waves share the attempts to wrap and measure the texts (every lane wraps the words of an
// attempt, lane k measures line k, the wave takes the widest); one wave then walks the 32 attempts in order -- lane r tests
// try r against the boxes accepted so far, one ballot picks the lowest accepted try -- and the waves write the lines and
// glyphs of the accepted attempts, lane k line k.  A dropped attempt writes nothing.
// Render: a block per tile of PG_TILE_H x PG_TILE_W pixels stages the paragraph boxes of its page, classifies its pixels
// into one 32-bit word each (coverage, id bits, flags; LDS) and writes the tile's rows of the five outputs from the words;
// where no box meets the tile it stores each layer's constant without a word in between.  Either way a row of a tile is
// one contiguous span of cols * C elements, 16-byte stores between a scalar head and tail.  Every element is written exactly once, by one thread; no memset, no atomics.
// Whatever the tables hold, a pixel only READS through them (every index is clamped to its table): hand-built tables
// cannot make the kernel write outside its outputs.
#include "entry_batch.h"

namespace {

constexpr int PG_ATTEMPTS = 32;            // paragraph attempts per page
constexpr int PG_MAX_WORDS = 30, PG_MAX_WORD = 10, PG_TRIES = 64;
constexpr int PG_MARGIN = 3, PG_LEFT = 20;
constexpr int PG_IDS = 162;                // character ids (0, the tab, is never drawn)
constexpr int PG_FACE_INTS = 7;            // size, ascent, descent, height, x_height, spacing, pitch
constexpr int PG_MAX_PAR = PG_ATTEMPTS;
constexpr int PG_MAX_LINES = PG_ATTEMPTS * PG_MAX_WORDS;
constexpr int PG_MAX_GLYPHS = PG_ATTEMPTS * PG_MAX_WORDS * (PG_MAX_WORD + 1);
constexpr int PG_PAR_INTS = 8, PG_LINE_INTS = 5, PG_GLYPH_INTS = 2, PG_COUNT_INTS = 4;
constexpr int PG_MAX_FACES = 256;
constexpr int PG_NT = 256;                 // threads of a render block
constexpr int PG_TILE_H = 16, PG_TILE_W = 32;
constexpr int PG_PAGES = 256;              // pages per launch
static_assert(PG_MAX_PAR * PG_PAR_INTS == PG_NT, "one thread stages one int of the paragraph table");
static_assert(PG_TRIES == UOCR_WAVE, "one lane per try");

__device__ __forceinline__ int pg_draw(uint64_t seed, uint64_t key, int slot, int lo, int hi) {
    uint64_t z = seed + (key + (uint64_t)slot + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return lo + (int)(((z >> 32) * (uint64_t)(hi - lo + 1)) >> 32);
}

// ---- layout: one block of PG_LAYOUT_WAVES waves per page ---------------------------------------------------------
// calls f(position in the line, id) for every glyph of the line made of words [first_word, first_word + words)
template <typename F>
__device__ __forceinline__ void pg_walk_line(uint64_t seed, uint64_t key, int first_word, int words, F f) {
    int at = 0;
    for (int w = 0; w < words; ++w) {
        const int j = first_word + w;
        const int len = pg_draw(seed, key, 3 + j, 1, PG_MAX_WORD);
        if (w > 0) f(at++, 1);
        for (int i = 0; i < len; ++i) f(at++, pg_draw(seed, key, 64 + PG_MAX_WORD * j + i, 2, PG_IDS - 1));
    }
}

// The text of an attempt as lane `lane` sees it: greedy wrapping, the same in every lane (30 draws at most); lane k keeps
// where line k starts.
struct PGText {
    int face, n_lines, total;            // total: glyphs of the paragraph
    int first_word, words, glyph0;       // of the lane's line: its first word, its words, the glyphs in front of it
};
__device__ __forceinline__ PGText pg_text(uint64_t seed, uint64_t key, int n_faces, int lane) {
    PGText t;
    t.face = pg_draw(seed, key, 0, 0, n_faces - 1);
    const int n_words = pg_draw(seed, key, 1, 3, PG_MAX_WORDS);
    const int wrap = pg_draw(seed, key, 2, 30, 100);
    int line = 0, cur = 0, before = 0;
    t.first_word = t.words = t.glyph0 = 0;
    for (int j = 0; j < n_words; ++j) {
        const int len = pg_draw(seed, key, 3 + j, 1, PG_MAX_WORD);
        if (j > 0 && cur + 1 + len <= wrap) {
            cur += 1 + len;
        } else {
            if (j > 0) before += cur, ++line;
            cur = len;
            if (line == lane) t.first_word = j, t.glyph0 = before;
        }
        t.words += line == lane;
    }
    t.n_lines = line + 1, t.total = before + cur;
    return t;
}

// Texts and sizes depend on no placement, so the waves of a block share the attempts of their page:
//   measure  wave w takes attempts w, w + PG_LAYOUT_WAVES, ..: lane k adds up line k, the wave keeps the widest (LDS)
//   place    wave 0 walks the attempts in order: lane r tests try r against the boxes accepted so far (lane q holds box q:
//            registers and shuffles, no LDS), one ballot picks the lowest accepted try; lane 0 writes the paragraph row
//   write    wave w writes the lines and glyphs of its accepted attempts, lane k line k.  A dropped attempt writes nothing.
constexpr int PG_LAYOUT_WAVES = 16;
static_assert(PG_MAX_WORDS <= UOCR_WAVE && PG_MAX_PAR <= UOCR_WAVE, "a lane per line, a lane per accepted box");

__global__ __launch_bounds__(PG_LAYOUT_WAVES * UOCR_WAVE) void page_layout_kernel(
    uint64_t seed, uint64_t first_page, int H, int W, int n_faces, const int* __restrict__ metrics,
    const int* __restrict__ adv, int* __restrict__ par, int* __restrict__ lines, int* __restrict__ glyphs,
    int* __restrict__ counts) {
    __shared__ int s_size[PG_ATTEMPTS][4];       // face, n_lines, glyphs, t_width
    __shared__ int s_place[PG_ATTEMPTS][4];      // x0, y0, first_line, first_glyph; x0 < 0: the attempt was dropped
    const int lane = threadIdx.x & (UOCR_WAVE - 1), wave = threadIdx.x / UOCR_WAVE;
    const uint64_t page = first_page + blockIdx.x;
    par += (size_t)blockIdx.x * PG_MAX_PAR * PG_PAR_INTS;
    lines += (size_t)blockIdx.x * PG_MAX_LINES * PG_LINE_INTS;
    glyphs += (size_t)blockIdx.x * PG_MAX_GLYPHS * PG_GLYPH_INTS;

    for (int attempt = wave; attempt < PG_ATTEMPTS; attempt += PG_LAYOUT_WAVES) {
        const uint64_t key = (page * PG_ATTEMPTS + (uint64_t)attempt) * 1024ull;
        const PGText t = pg_text(seed, key, n_faces, lane);
        const int* fadv = adv + t.face * PG_IDS;
        int width = 0;
        if (lane < t.n_lines) pg_walk_line(seed, key, t.first_word, t.words, [&](int, int id) { width += fadv[id]; });
        width = wave_reduce_max(width);
        if (lane == 0) s_size[attempt][0] = t.face, s_size[attempt][1] = t.n_lines, s_size[attempt][2] = t.total, s_size[attempt][3] = width;
    }
    __syncthreads();

    if (wave == 0) {
        int n_par = 0, n_line = 0, n_glyph = 0;
        int bx = 0, by = 0, bw = 0, bh = 0;      // lane q: the box of accepted paragraph q
        for (int attempt = 0; attempt < PG_ATTEMPTS; ++attempt) {
            const uint64_t key = (page * PG_ATTEMPTS + (uint64_t)attempt) * 1024ull;
            const int face = s_size[attempt][0], n_lines = s_size[attempt][1], total = s_size[attempt][2], t_width = s_size[attempt][3];
            const int spacing = metrics[face * PG_FACE_INTS + 5], pitch = metrics[face * PG_FACE_INTS + 6];
            const int t_height = n_lines * pitch - spacing;
            const int pw = t_width + 2 * PG_MARGIN, ph = t_height + 2 * PG_MARGIN;
            const int x_hi = W - pw - PG_LEFT, y_hi = H - ph;
            unsigned long long accepted = 0;
            int x = 0, y = 0;
            if (x_hi >= PG_LEFT && y_hi >= 0) {                  // (wave-uniform) else: too large for the page
                x = pg_draw(seed, key, 512 + 2 * lane, PG_LEFT, x_hi), y = pg_draw(seed, key, 513 + 2 * lane, 0, y_hi);
                bool ok = true;
                for (int q = 0; q < n_par; ++q) {
                    const int qx = __shfl(bx, q, UOCR_WAVE), qy = __shfl(by, q, UOCR_WAVE);
                    const int qw = __shfl(bw, q, UOCR_WAVE), qh = __shfl(bh, q, UOCR_WAVE);
                    ok = ok && !(x < qx + qw && qx < x + pw && y < qy + qh && qy < y + ph);
                }
                accepted = __ballot(ok);
            }
            if (!accepted) {                                     // (wave-uniform) no room in 64 tries either
                if (lane == 0) s_place[attempt][0] = -1;
                continue;
            }
            const int winner = __ffsll(accepted) - 1;
            const int x0 = __shfl(x, winner, UOCR_WAVE) + PG_MARGIN, y0 = __shfl(y, winner, UOCR_WAVE) + PG_MARGIN;
            if (lane == n_par) bx = x0, by = y0, bw = t_width, bh = t_height;
            if (lane == 0) {
                int* p = par + n_par * PG_PAR_INTS;
                *reinterpret_cast<int4*>(p) = make_int4(x0, y0, t_width, t_height);
                *reinterpret_cast<int4*>(p + 4) = make_int4(face, n_lines, n_line, attempt);
                s_place[attempt][0] = x0, s_place[attempt][1] = y0, s_place[attempt][2] = n_line, s_place[attempt][3] = n_glyph;
            }
            ++n_par, n_line += n_lines, n_glyph += total;
        }
        if (lane == 0)
            *reinterpret_cast<int4*>(counts + (size_t)blockIdx.x * PG_COUNT_INTS) = make_int4(n_par, n_line, n_glyph, 0);
    }
    __syncthreads();

    for (int attempt = wave; attempt < PG_ATTEMPTS; attempt += PG_LAYOUT_WAVES) {
        const int x0 = s_place[attempt][0], y0 = s_place[attempt][1], n_line = s_place[attempt][2], n_glyph = s_place[attempt][3];
        if (x0 < 0) continue;                                    // (wave-uniform)
        const uint64_t key = (page * PG_ATTEMPTS + (uint64_t)attempt) * 1024ull;
        const PGText t = pg_text(seed, key, n_faces, lane);
        if (lane >= t.n_lines) continue;
        const int* fadv = adv + t.face * PG_IDS;
        const int pitch = metrics[t.face * PG_FACE_INTS + 6];
        int2* g = reinterpret_cast<int2*>(glyphs) + n_glyph + t.glyph0;
        int pen = x0, count = 0;
        pg_walk_line(seed, key, t.first_word, t.words, [&](int at, int id) { g[at] = make_int2(pen, id), pen += fadv[id], ++count; });
        int* l = lines + (size_t)(n_line + lane) * PG_LINE_INTS;
        l[0] = x0, l[1] = y0 + lane * pitch, l[2] = pen - x0, l[3] = n_glyph + t.glyph0, l[4] = count;
    }
}

// ---- render: one block per tile ------------------------------------------------------------------------------------
// the word of a pixel: bits 0-7 coverage, 8-15 the id inside its full box, 16 paragraph, 17 line_top, 18 line_bottom,
// 19 letter_spacing
constexpr unsigned PG_PARAGRAPH = 1u << 16, PG_TOP = 1u << 17, PG_BOTTOM = 1u << 18, PG_SPACING = 1u << 19;

struct PGRender {
    const int *par, *lines, *glyphs, *counts;      // of the first page of the launch
    const int *metrics, *adv, *offset;
    const unsigned char* cells;
    long long n_cells;
    const void* lut;
    void* out[5];                                  // image, monochrome, paragraph, line, char: the first page of the launch
    int H, W, n_faces, tiles_x, tiles_y;
};

// what the tables say about pixel (y, x) of paragraph row `b` (8 ints) of page tables (lines, glyphs)
__device__ __forceinline__ unsigned pg_classify(const PGRender& a, const int* b, const int* lines, const int* glyphs, int y,
                                                int x) {
    unsigned word = PG_PARAGRAPH;
    const int face = min(max(b[4], 0), a.n_faces - 1);
    const int* fm = a.metrics + face * PG_FACE_INTS;
    const int ascent = fm[1], height = fm[3], x_height = fm[4], pitch = max(fm[6], 1);
    const int k = (y - b[1]) / pitch, r = (y - b[1]) - k * pitch;
    if (k >= b[5] || r >= height || b[6] < 0 || b[6] >= PG_MAX_LINES || k >= PG_MAX_LINES - b[6]) return word;
    const int* l = lines + (size_t)(b[6] + k) * PG_LINE_INTS;
    const int left = l[0], width = l[2], g0 = l[3], ng = l[4];
    if (x < left || (long long)x - left >= width) return word;
    word |= (r < ascent ? PG_TOP : 0u) | (r >= ascent - x_height ? PG_BOTTOM : 0u);
    if (ng < 1 || g0 < 0 || g0 > PG_MAX_GLYPHS - ng) return word;
    const int2* g = reinterpret_cast<const int2*>(glyphs) + g0;
    int lo = 0, hi = ng;                           // the last glyph whose pen is not right of x
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g[mid].x <= x) lo = mid;
        else hi = mid;
    }
    const int2 glyph = g[lo];
    const int u = x - glyph.x, id = glyph.y;
    if (u < 0 || id < 1 || id >= PG_IDS) return word;
    const int* fadv = a.adv + face * PG_IDS;
    const int cell_w = fadv[id];
    if (u >= cell_w) return word;
    const int w10 = max(1, cell_w / 10);
    if (u >= w10 && u < cell_w - w10) word |= (unsigned)id << 8;
    if (lo < ng - 1 && u >= cell_w - w10) word |= PG_SPACING;
    if (lo > 0) {
        const int before = g[lo - 1].y;
        if (before >= 1 && before < PG_IDS && u < max(1, fadv[before] / 10)) word |= PG_SPACING;
    }
    const long long at = (long long)a.offset[face * PG_IDS + id] + (long long)r * cell_w + u;
    if (at >= 0 && at < a.n_cells) word |= a.cells[at];
    return word;
}

// rows x cols pixels of C channels from `out` on (rows `row_stride` elements apart): element (row, col, ch) =
// value(row, col, ch).  A row is a span of cols * C elements: slot 0 of a row is its scalar head, slots 1 .. nvec its
// 16-byte vectors, slot nvec + 1 its scalar tail; the slots of all rows are dealt to the threads.
template <typename T, int C, typename F>
__device__ __forceinline__ void pg_store(T* out, size_t row_stride, int rows, int cols, F value) {
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    const int span = cols * C, slots = span / VEC + 2;
    for (int i = threadIdx.x; i < rows * slots; i += PG_NT) {
        const int row = i / slots, slot = i - row * slots;
        T* p = out + row * row_stride;
        const auto [head, nvec, tail] = eb_split(p, span);
        if (slot == 0) {
            for (int e = 0; e < head; ++e) p[e] = value(row, e / C, e % C);
        } else if (slot <= nvec) {
            const int e0 = head + (slot - 1) * VEC;
            V v;
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = value(row, (e0 + j) / C, (e0 + j) % C);
            *reinterpret_cast<V*>(p + e0) = v;
        } else if (slot == nvec + 1) {
            for (int e = span - tail; e < span; ++e) p[e] = value(row, e / C, e % C);
        }
    }
}

// the tile's rows of the five outputs from the words of its pixels, word(row, col)
template <typename T, typename W>
__device__ __forceinline__ void pg_store_layers(const PGRender& a, size_t first, int rows, int cols, const T* s_lut, W word) {
    const auto flag = [](unsigned w, int bit) { return (T)(float)((w >> bit) & 1u); };
    pg_store<T, 1>(static_cast<T*>(a.out[0]) + first, (size_t)a.W, rows, cols,
                   [&](int row, int col, int) { return s_lut[255 - (word(row, col) & 255u)]; });
    pg_store<T, 1>(static_cast<T*>(a.out[1]) + first, (size_t)a.W, rows, cols,
                   [&](int row, int col, int) { return s_lut[word(row, col) & 255u]; });
    pg_store<T, 1>(static_cast<T*>(a.out[2]) + first, (size_t)a.W, rows, cols,
                   [&](int row, int col, int) { return flag(word(row, col), 16); });
    pg_store<T, 2>(static_cast<T*>(a.out[3]) + first * 2, (size_t)a.W * 2, rows, cols,
                   [&](int row, int col, int ch) { return flag(word(row, col), 17 + ch); });
    pg_store<T, 9>(static_cast<T*>(a.out[4]) + first * 9, (size_t)a.W * 9, rows, cols,
                   [&](int row, int col, int ch) { return flag(word(row, col), ch < 8 ? 8 + ch : 19); });
}

template <typename T>
__global__ __launch_bounds__(PG_NT) void page_render_kernel(const PGRender a) {
    __shared__ int s_box[PG_MAX_PAR * PG_PAR_INTS];
    __shared__ int s_hit;
    __shared__ unsigned s_word[PG_TILE_H * PG_TILE_W];
    __shared__ T s_lut[256];
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int page = blockIdx.x / tiles, tile = blockIdx.x - page * tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int r0 = ty * PG_TILE_H, c0 = tx * PG_TILE_W;
    const int rows = min(PG_TILE_H, a.H - r0), cols = min(PG_TILE_W, a.W - c0);
    const int n = min(max(a.counts[(size_t)page * PG_COUNT_INTS], 0), PG_MAX_PAR);
    static_assert(PG_NT == 256, "one thread per entry of the lut");
    s_lut[tid] = static_cast<const T*>(a.lut)[tid];
    if (tid < n * PG_PAR_INTS) s_box[tid] = a.par[(size_t)page * PG_MAX_PAR * PG_PAR_INTS + tid];
    if (tid == 0) s_hit = 0;
    __syncthreads();
    if (tid < n) {
        const int* b = s_box + tid * PG_PAR_INTS;
        if (b[0] < c0 + cols && c0 < (long long)b[0] + b[2] && b[1] < r0 + rows && r0 < (long long)b[1] + b[3]) s_hit = 1;
    }
    __syncthreads();
    const size_t first = ((size_t)page * a.H + r0) * a.W + c0;
    if (s_hit) {                                                 // (block-uniform)
        const int* lines = a.lines + (size_t)page * PG_MAX_LINES * PG_LINE_INTS;
        const int* glyphs = a.glyphs + (size_t)page * PG_MAX_GLYPHS * PG_GLYPH_INTS;
        for (int i = tid; i < PG_TILE_H * PG_TILE_W; i += PG_NT) {
            const int ly = i / PG_TILE_W, lx = i % PG_TILE_W, y = r0 + ly, x = c0 + lx;
            unsigned word = 0;
            if (ly < rows && lx < cols)                          // (a tile on the page's edge: nobody reads the rest)
                for (int q = 0; q < n; ++q) {                    // the first box that holds the pixel owns it
                    const int* b = s_box + q * PG_PAR_INTS;
                    if (x >= b[0] && x - b[0] < b[2] && y >= b[1] && y - b[1] < b[3]) {
                        word = pg_classify(a, b, lines, glyphs, y, x);
                        break;
                    }
                }
            s_word[i] = word;
        }
        __syncthreads();
        pg_store_layers<T>(a, first, rows, cols, s_lut, [&](int row, int col) { return s_word[row * PG_TILE_W + col]; });
    } else {                                                     // blank paper: every value is a constant of its layer
        pg_store_layers<T>(a, first, rows, cols, s_lut, [](int, int) { return 0u; });
    }
}

bool pg_aligned(const void* p, size_t elem) { return reinterpret_cast<uintptr_t>(p) % elem == 0; }

}  // namespace

extern "C" {

int uocr_page_layout(uocr_ctx* ctx, unsigned long long seed, unsigned long long first_page, int n_pages, int height,
                     int width, int n_faces, const int* metrics, const int* adv, int* paragraphs, int* lines, int* glyphs,
                     int* counts) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_pages >= 0);
    if (n_pages == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, metrics && adv && paragraphs && lines && glyphs && counts);
    UOCR_REQUIRE(ctx, height >= 1 && width >= 1 && height <= (1 << 24) && width <= (1 << 24));
    UOCR_REQUIRE(ctx, n_faces >= 1 && n_faces <= PG_MAX_FACES);
    UOCR_REQUIRE(ctx, pg_aligned(metrics, 4) && pg_aligned(adv, 4) && pg_aligned(lines, 4));
    UOCR_REQUIRE(ctx, pg_aligned(paragraphs, 16) && pg_aligned(glyphs, 8) && pg_aligned(counts, 16));
    int launches = 0;
    for (int first = 0; first < n_pages; first += PG_PAGES, ++launches) {
        const int count = eb_group_size(n_pages, first, PG_PAGES);
        hipLaunchKernelGGL(page_layout_kernel, dim3((unsigned)count), dim3(PG_LAYOUT_WAVES * UOCR_WAVE), 0, ctx->stream, (uint64_t)seed,
                           (uint64_t)first_page + (uint64_t)first, height, width, n_faces, metrics, adv,
                           paragraphs + (size_t)first * PG_MAX_PAR * PG_PAR_INTS, lines + (size_t)first * PG_MAX_LINES * PG_LINE_INTS,
                           glyphs + (size_t)first * PG_MAX_GLYPHS * PG_GLYPH_INTS, counts + (size_t)first * PG_COUNT_INTS);
        UOCR_LAUNCH_CHECK(ctx);
    }
    uocr_note(ctx, UOCR_REPORT_PAGE_GEN, PG_TILE_H, PG_TILE_W, PG_PAGES, launches);
    return UOCR_OK;
}

int uocr_page_render(uocr_ctx* ctx, int dtype, int n_pages, int height, int width, const int* paragraphs, const int* lines,
                     const int* glyphs, const int* counts, int n_faces, const int* metrics, const int* adv, const int* offset,
                     const unsigned char* cells, long long n_cells, const void* lut, void* image, void* monochrome,
                     void* paragraph, void* line, void* chr) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_pages >= 0);
    if (n_pages == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, paragraphs && lines && glyphs && counts && metrics && adv && offset && cells && lut);
    UOCR_REQUIRE(ctx, image && monochrome && paragraph && line && chr);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    UOCR_REQUIRE(ctx, height >= 1 && width >= 1 && height <= (1 << 24) && width <= (1 << 24));
    UOCR_REQUIRE(ctx, n_faces >= 1 && n_faces <= PG_MAX_FACES && n_cells >= 0);
    UOCR_REQUIRE(ctx, pg_aligned(paragraphs, 4) && pg_aligned(lines, 4) && pg_aligned(glyphs, 8) && pg_aligned(counts, 4));
    UOCR_REQUIRE(ctx, pg_aligned(metrics, 4) && pg_aligned(adv, 4) && pg_aligned(offset, 4) && pg_aligned(lut, elem));
    void* const outs[5] = {image, monochrome, paragraph, line, chr};
    const int channels[5] = {1, 1, 1, 2, 9};
    for (void* out : outs) UOCR_REQUIRE(ctx, pg_aligned(out, elem));
    const int tiles_x = (width + PG_TILE_W - 1) / PG_TILE_W, tiles_y = (height + PG_TILE_H - 1) / PG_TILE_H;
    const long long tiles = (long long)tiles_x * tiles_y;
    if (tiles > INT32_MAX) UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "a page of %d x %d has too many tiles for one grid", height, width);
    const int per_launch = (int)(INT32_MAX / tiles < PG_PAGES ? INT32_MAX / tiles : PG_PAGES);
    int launches = 0;
    for (int first = 0; first < n_pages; first += per_launch, ++launches) {
        const int count = eb_group_size(n_pages, first, per_launch);
        PGRender a;
        a.par = paragraphs + (size_t)first * PG_MAX_PAR * PG_PAR_INTS, a.lines = lines + (size_t)first * PG_MAX_LINES * PG_LINE_INTS;
        a.glyphs = glyphs + (size_t)first * PG_MAX_GLYPHS * PG_GLYPH_INTS, a.counts = counts + (size_t)first * PG_COUNT_INTS;
        a.metrics = metrics, a.adv = adv, a.offset = offset, a.cells = cells, a.n_cells = n_cells, a.lut = lut;
        for (int o = 0; o < 5; ++o)
            a.out[o] = static_cast<char*>(outs[o]) + (size_t)first * height * width * channels[o] * elem;
        a.H = height, a.W = width, a.n_faces = n_faces, a.tiles_x = tiles_x, a.tiles_y = tiles_y;
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL(page_render_kernel<T>, dim3((unsigned)(tiles * count)), dim3(PG_NT), 0, ctx->stream, a);
            UOCR_LAUNCH_CHECK(ctx);
        });
    }
    uocr_note(ctx, UOCR_REPORT_PAGE_GEN, PG_TILE_H, PG_TILE_W, per_launch, launches);
    return UOCR_OK;
}

int uocr_ctx_last_page_gen(uocr_ctx* ctx, int* tile_rows, int* tile_cols, int* pages_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_PAGE_GEN, tile_rows, tile_cols, pages_per_launch, launches);
}

}  // extern "C"
