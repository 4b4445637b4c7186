// Annotated frames behind the decode, the plate crops and the tracking update: what the reference's viz_result (DenseBox.py:3484-3560)
// draws with OpenCV -- the box, a filled label with the score, four landmark discs, the rectified plate next to the box -- painted on the
// device by ONE launch (dbx_draw_overlay_batch).  The layout, default colours, thickness, radius and anchor points follow viz_result; the
// pixel semantics are this project's own (include/densebox_hip.h states them, tests/viz_ref.py restates them in NumPy) and parity with
// cv2.rectangle / putText / circle is unpinned: OpenCV is not part of the reference tree.  Every pixel is a function of the inputs
// alone: integer arithmetic behind one float64 add per coordinate.
#include "common.hpp"
#include "det_frame.hpp"
#include "frame_tile.hpp"

#define VIZ_TW 128                   // a tile: 128 x 16 pixels, 8 per thread; the copy moves a row segment with 32 lanes
#define VIZ_TH 16
#define VIZ_MAX_SLOTS 1024
#define VIZ_MAX_LABEL 21             // "#2147483647 " + "-1000.000"

// ---------------------------------------------------------------------------------------------------------------- font and text
// The 14 glyphs of "0123456789.-# ", 5 x 7 in a 6 x 8 cell: byte j of a word is row j, bit i of a byte column i (column 5 and row 7
// stay empty).
__host__ __device__ static inline unsigned long long viz_glyph(int g) {
    const unsigned long long font[14] = {
        0x000E11131519110Eull, 0x000E040404040604ull, 0x001F02040810110Eull, 0x000E11100C10110Eull, 0x0008081F090A0C08ull,     // 0 1 2 3 4
        0x000E1110100F011Full, 0x000E11110F01020Cull, 0x000202020408101Full, 0x000E11110E11110Eull, 0x000608101E11110Eull,     // 5 6 7 8 9
        0x0006060000000000ull, 0x000000001F000000ull, 0x000A0A1F0A1F0A0Aull, 0x0000000000000000ull};                           // . - # space
    return font[g];
}

// A label as glyph numbers, four bits each, in two words (no array: nothing spills), and its length.
struct VizLabel { unsigned long long lo, hi; int n; };
__host__ __device__ static inline void viz_put(VizLabel& t, int g) {
    if (t.n < 16) t.lo |= (unsigned long long)g << (4 * t.n);
    else t.hi |= (unsigned long long)g << (4 * (t.n - 16));
    ++t.n;
}
__host__ __device__ static inline int viz_get(unsigned long long lo, unsigned long long hi, int m) {
    return (int)((m < 16 ? lo >> (4 * m) : hi >> (4 * (m - 16))) & 15ull);
}
__host__ __device__ static inline void viz_put_uint(VizLabel& t, unsigned v) {
    unsigned pw = 1;
    while (v / pw >= 10) pw *= 10;
    for (; pw; pw /= 10) viz_put(t, (int)(v / pw % 10));
}
// "#<id> " when id >= 0, then the score as '%.3f' prints it, from the double's bits: |v| = M * 2^-sh with M < 2^53 and, below 1000,
// sh >= 43; M * 1000 < 2^63, its quotient by 2^sh rounded to nearest, ties to even, is the number of thousandths.  Not finite or
// |v| >= 1000: "---".
__host__ __device__ static inline VizLabel viz_label(unsigned long long bits, int id) {
    VizLabel t;
    t.lo = t.hi = 0ull; t.n = 0;
    if (id >= 0) { viz_put(t, 12); viz_put_uint(t, (unsigned)id); viz_put(t, 13); }
    const unsigned long long mag = bits & 0x7fffffffffffffffull;
    if (mag >= 0x408F400000000000ull) {                            // 1000.0, and every infinity and NaN above it
        viz_put(t, 11); viz_put(t, 11); viz_put(t, 11);
        return t;
    }
    const int e = (int)(mag >> 52);
    const unsigned long long man = mag & 0x000fffffffffffffull;
    const unsigned long long M = e ? man | 0x0010000000000000ull : man;
    const int sh = e ? 1075 - e : 1074;
    const unsigned long long P = M * 1000ull;
    unsigned long long q = 0;
    if (sh < 64) {
        q = P >> sh;
        const unsigned long long rem = P & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
        if (rem > half || (rem == half && (q & 1ull))) ++q;
    }
    if (bits >> 63) viz_put(t, 11);
    viz_put_uint(t, (unsigned)(q / 1000ull));
    viz_put(t, 10);
    const unsigned fr = (unsigned)(q % 1000ull);
    viz_put(t, (int)(fr / 100)); viz_put(t, (int)(fr / 10 % 10)); viz_put(t, (int)(fr % 10));
    return t;
}

extern "C" int dbx_overlay_font(uint8_t* out) {
    DBX_REQUIRE(out, "overlay_font: null argument");
    for (int g = 0; g < 14; ++g)
        for (int j = 0; j < 8; ++j) out[g * 8 + j] = (uint8_t)(viz_glyph(g) >> (8 * j));
    return DBX_OK;
}

extern "C" int dbx_overlay_label(double score, int32_t track_id, char* out, int32_t out_len) {
    DBX_REQUIRE(out && out_len > VIZ_MAX_LABEL, "overlay_label: out must hold %d characters and the terminator", VIZ_MAX_LABEL);
    unsigned long long bits;
    __builtin_memcpy(&bits, &score, 8);
    const VizLabel t = viz_label(bits, track_id);
    for (int m = 0; m < t.n; ++m) out[m] = "0123456789.-# "[viz_get(t.lo, t.hi, m)];
    out[t.n] = 0;
    return t.n;
}

// ---------------------------------------------------------------------------------------------------------------- the kernel
struct VizArgs {
    const dbx_overlay_frame* frames; const double* dets; const int* keep; const int* prefix; const int* track_id;
    const uint8_t* crops; const int* ok;
    long long det_rows;
    dbx_overlay_style st;
    int c, det_cols, slots, ow, oh, tiles_x, max_h, max_w;
};

// A kept row as the pixels test it: 88 bytes of LDS.  word: the list position (bits 0..9), the label's length (10..14), discs 0..3
// drawn (15..18), inset drawn (19).  bx0..by1: the bounding rectangle of everything the row paints, clamped to 32 bits.
struct VizEnt { unsigned long long tlo, thi; int x1, y1, x2, y2; int cx[4], cy[4]; int word, pad; int bx0, bx1, by0, by1; };
static size_t viz_lds_bytes(int slots) { return ((size_t)slots * sizeof(VizEnt) + 15) & ~(size_t)15; }

// Row d at list position i of frame b as entry e, and the bounding rectangle box = (x min, x max, y min, y max) of everything it
// paints (with the longest label; viz_entry_label makes the text); false when the row paints nothing.
__host__ __device__ static inline bool viz_entry(const VizArgs& a, int b, int i, const double* d, VizEnt& e, long long* box) {
    const double bx1 = d[0], by1 = d[1], bx2 = d[2], by2 = d[3];
    if (!(tile_usable(bx1) && tile_usable(by1) && tile_usable(bx2) && tile_usable(by2))) return false;
    const int ta = a.st.thickness / 2, s = a.st.font_scale, rad = a.st.radius;
    e.x1 = (int)(bx1 + 0.5); e.y1 = (int)(by1 + 0.5); e.x2 = (int)(bx2 + 0.5); e.y2 = (int)(by2 + 0.5);
    const int L = tile_min(e.x1, e.x2), R = tile_max(e.x1, e.x2), Tp = tile_min(e.y1, e.y2), Bt = tile_max(e.y1, e.y2);
    long long xa = L - ta, xb = R + ta, ya = Tp - ta, yb = Bt + ta;
    int word = i;
    e.tlo = e.thi = 0ull; e.pad = 0;
    if (s > 0) {                                                   // (the longest label: the text is made by viz_entry_label, for the rows a tile keeps)
        xa = tile_min(xa, (long long)e.x1); xb = tile_max(xb, (long long)e.x1 + 6 * s * VIZ_MAX_LABEL + 3);
        ya = tile_min(ya, (long long)e.y1 - 8 * s - 5); yb = tile_max(yb, (long long)e.y1);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        e.cx[q] = e.cy[q] = 0;
        if (a.det_cols != 13 || rad < 0) continue;
        const double px = d[5 + 2 * q], py = d[6 + 2 * q];
        if (!tile_usable(px) || !tile_usable(py)) continue;
        e.cx[q] = (int)px; e.cy[q] = (int)py;
        word |= 1 << (15 + q);
        xa = tile_min(xa, (long long)e.cx[q] - rad); xb = tile_max(xb, (long long)e.cx[q] + rad);
        ya = tile_min(ya, (long long)e.cy[q] - rad); yb = tile_max(yb, (long long)e.cy[q] + rad);
    }
    if (a.crops && a.ok[(size_t)b * a.slots + i] != 0) {
        word |= 1 << 19;
        const long long px = L - ta, py = (long long)Bt + ta + 2;
        xa = tile_min(xa, px); xb = tile_max(xb, px + (long long)a.ow * a.st.inset_scale - 1);
        ya = tile_min(ya, py); yb = tile_max(yb, py + (long long)a.oh * a.st.inset_scale - 1);
    }
    e.word = word;
    box[0] = xa; box[1] = xb; box[2] = ya; box[3] = yb;
    const long long lo = -2147483647ll - 1, hi = 2147483647ll;
    e.bx0 = (int)tile_max(xa, lo); e.bx1 = (int)tile_min(xb, hi); e.by0 = (int)tile_max(ya, lo); e.by1 = (int)tile_min(yb, hi);
    return true;
}

// The label of the row viz_entry made e from: its glyphs and its length.
__host__ __device__ static inline void viz_entry_label(const VizArgs& a, int b, int i, const double* d, VizEnt& e) {
    if (a.st.font_scale <= 0) return;
    const int id = a.track_id ? a.track_id[(size_t)b * a.slots + i] : -1;
    const VizLabel lab = viz_label(__builtin_bit_cast(unsigned long long, d[4]), id);
    e.tlo = lab.lo; e.thi = lab.hi;
    e.word |= lab.n << 10;
}

// What row e paints at (x, y), its primitives tried from the last painted to the first: 0 nothing, 1 box colour, 2 text colour, 3 mark
// colour, 4 the crop pixel *cp.
__host__ __device__ static inline int viz_hit(const VizEnt& e, const VizArgs& a, int b, int x, int y, const uint8_t** cp) {
    if (x < e.bx0 || x > e.bx1 || y < e.by0 || y > e.by1) return 0;
    const int t = a.st.thickness, ta = t / 2, tb = t - ta, s = a.st.font_scale, w = e.word;
    const int L = tile_min(e.x1, e.x2), R = tile_max(e.x1, e.x2), Tp = tile_min(e.y1, e.y2), Bt = tile_max(e.y1, e.y2);
    if (w & (1 << 19)) {
        const long long m = a.st.inset_scale, dx = (long long)x - (L - ta), dy = (long long)y - (Bt + ta + 2);
        if (dx >= 0 && dy >= 0 && dx < a.ow * m && dy < a.oh * m) {
            *cp = a.crops + ((((size_t)b * a.slots + (w & 1023)) * a.oh + (size_t)(dy / m)) * a.ow + (size_t)(dx / m)) * a.c;
            return 4;
        }
    }
    const long long r2 = (long long)a.st.radius * a.st.radius;
#pragma unroll
    for (int q = 3; q >= 0; --q) {
        if (!(w & (1 << (15 + q)))) continue;
        const long long dx = (long long)x - e.cx[q], dy = (long long)y - e.cy[q];
        if (dx * dx + dy * dy <= r2) return 3;
    }
    if (s > 0) {
        const int n = (w >> 10) & 31, tw = 6 * s * n, th = 8 * s;
        if (x >= e.x1 && x <= e.x1 + tw + 3 && y >= e.y1 - th - 5 && y <= e.y1) {
            const int u = x - (e.x1 + 2), v = y - (e.y1 - 2 - th);
            if (u >= 0 && u < tw && v >= 0 && v < th) {
                const int m = u / (6 * s), i = (u - m * 6 * s) / s, j = v / s;
                if ((viz_glyph(viz_get(e.tlo, e.thi, m)) >> (8 * j + i)) & 1ull) return 2;
            }
            return 1;
        }
    }
    if (x >= L - ta && x <= R + ta && y >= Tp - ta && y <= Bt + ta && !(x >= L + tb && x <= R - tb && y >= Tp + tb && y <= Bt - tb)) return 1;
    return 0;
}

// One workgroup per 128 x 16 tile of a frame (grid: the tiles of a max_h x max_w frame, batch), walked as frame_tile.hpp says.  The
// candidates are the frame's kept rows, and a row meets the tile when the bounding rectangle of its primitives does; the list keeps
// list order.  A pixel is resolved by walking the list from the back to the first row that paints it.
__global__ __launch_bounds__(TILE_THREADS) void draw_overlay_batch_kernel(const VizArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char viz_sm[];
    VizEnt* list = (VizEnt*)viz_sm;
    const int b = blockIdx.y, c = a.c;
    FrameTile t;
    if (!tile_open<VIZ_TW, VIZ_TH>(a.frames, a.tiles_x, a.max_h, a.max_w, t)) return;              // uniform, as the return below
    unsigned cbox, ctext, cmark;                                   // colour[ch] in byte ch
    __builtin_memcpy(&cbox, a.st.box_color, 4); __builtin_memcpy(&ctext, a.st.text_color, 4); __builtin_memcpy(&cmark, a.st.mark_color, 4);

    const DetFrame fr = det_frame(a.keep, a.prefix, b, a.slots, a.det_rows);
    const int cnt = tile_collect(list, fr.k, [&](int i, VizEnt& e) {
        const int r = fr.kl[1 + i];
        if (r < 0 || r >= fr.n) return false;
        const double* d = a.dets + (size_t)(fr.r0 + r) * a.det_cols;
        long long box[4];
        if (!viz_entry(a, b, i, d, e, box) || !tile_meets(t, box[0], box[1], box[2], box[3])) return false;
        viz_entry_label(a, b, i, d, e);
        return true;
    });
    if (cnt == 0) {
        tile_copy_through<VIZ_TW>(t, c);
        return;
    }
    // The pixels, by a loop of the kernel's own, as in redact_ops.hip: a shared skeleton that took the painting as a lambda cost the
    // redaction's blur 0.8 % (profiles/r21_frame_tile.txt) and would have had this kernel as its only user.
    const dbx_overlay_frame fm = t.fm;
    const bool copying = fm.dst != fm.src;
    for (int p = threadIdx.x; p < VIZ_TW * VIZ_TH; p += TILE_THREADS) {
        const int lx = p & (VIZ_TW - 1), ly = p / VIZ_TW;
        if (lx >= t.cols || ly >= t.rows) continue;
        const int x = t.x0 + lx, y = t.y0 + ly;
        int kind = 0;
        const uint8_t* cp = nullptr;
        for (int k = cnt - 1; k >= 0 && !kind; --k) kind = viz_hit(list[k], a, b, x, y, &cp);
        const size_t o = ((size_t)y * fm.w + x) * c;
        if (kind == 0) {
            for (int ch = 0; copying && ch < c; ++ch) fm.dst[o + ch] = fm.src[o + ch];
            continue;
        }
        const unsigned col = kind == 1 ? cbox : (kind == 2 ? ctext : cmark);
        for (int ch = 0; ch < c; ++ch) fm.dst[o + ch] = kind == 4 ? cp[ch] : (uint8_t)(col >> (8 * ch));
    }
}

extern "C" int dbx_draw_overlay_batch(const dbx_overlay_frame* frames, int32_t batch, int32_t c, int32_t max_h, int32_t max_w,
                                      const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                                      int32_t slots, const int32_t* track_id, const uint8_t* crops, const int32_t* ok, int32_t ow, int32_t oh,
                                      const dbx_overlay_style* style, void* stream) {
    static_assert(sizeof(dbx_overlay_frame) == 24 && sizeof(dbx_overlay_style) == 28, "dbx_overlay_frame is 24 bytes, dbx_overlay_style 28");
    static_assert(sizeof(VizEnt) == 88, "a collected row is 88 bytes of LDS");
    const char* fn = "draw_overlay_batch";
    int rc = det_rows_check(fn, det_cols, det_rows, prefix, batch, slots, VIZ_MAX_SLOTS);
    if (rc == DBX_OK) rc = tile_dims_check(fn, c, max_h, max_w);
    if (rc != DBX_OK) return rc;
    DBX_REQUIRE(style, "%s: null style", fn);
    DBX_REQUIRE(style->thickness >= 1 && style->thickness <= 16, "%s: thickness=%d must be 1..16", fn, style->thickness);
    DBX_REQUIRE(style->radius >= -1 && style->radius <= 32, "%s: radius=%d must be -1..32", fn, style->radius);
    DBX_REQUIRE(style->font_scale >= 0 && style->font_scale <= 8, "%s: font_scale=%d must be 0..8", fn, style->font_scale);
    DBX_REQUIRE(style->inset_scale >= 1 && style->inset_scale <= 8, "%s: inset_scale=%d must be 1..8", fn, style->inset_scale);
    DBX_REQUIRE((crops == nullptr) == (ok == nullptr), "%s: crops and ok must be given together", fn);
    DBX_REQUIRE(!crops || (ow >= 1 && oh >= 1), "%s: a crop of %d x %d pixels is empty", fn, ow, oh);
    DBX_REQUIRE(frames && dets && keep, "%s: null argument", fn);
    VizArgs a;
    dim3 grid;
    rc = tile_grid<VIZ_TW, VIZ_TH>(fn, max_h, max_w, batch, &grid, &a.tiles_x);
    if (rc != DBX_OK || batch == 0) return rc;
    const size_t lds = viz_lds_bytes(slots);
    rc = tile_lds_limit<draw_overlay_batch_kernel>(lds, viz_lds_bytes(VIZ_MAX_SLOTS));
    if (rc != DBX_OK) return rc;
    a.frames = frames; a.dets = dets; a.keep = keep; a.prefix = prefix; a.track_id = track_id; a.crops = crops; a.ok = ok;
    a.det_rows = det_rows; a.st = *style; a.c = c; a.det_cols = det_cols; a.slots = slots; a.ow = ow; a.oh = oh;
    a.max_h = max_h; a.max_w = max_w;
    hipLaunchKernelGGL(draw_overlay_batch_kernel, grid, dim3(TILE_THREADS), lds, (hipStream_t)stream, a);
    DBX_LAUNCH_CHECK();
    return DBX_OK;
}
