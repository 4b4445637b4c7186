// The description of a batch of decoded rows as the decodes leave them on the device -- dets, det_cols, det_rows, keep, prefix, batch,
// slots, in the slot layout of dbx_detect_batch (prefix == NULL) or the packed layout of dbx_detect_thresh_batch -- shared by every
// entry point that takes it and every kernel that walks the kept rows: eval_ops.hip (dbx_match_gt_batch, dbx_eval_append),
// track_ops.hip (dbx_track_update_batch), viz_ops.hip (dbx_draw_overlay_batch) and redact_ops.hip (dbx_redact_batch).  Integer
// arithmetic only, and it has to stay so: eval_ops.hip and track_ops.hip compile with `#pragma clang fp contract(off)`, viz_ops.hip and
// redact_ops.hip without, which makes no difference here.
#pragma once
#include "common.hpp"

// Where frame b's rows and keep list are, from device data that is never trusted as a bound: r0 the frame's first row of dets, n its
// rows, kl its keep list (the count, then row numbers within the frame), k the clamped count.  A frame of the packed layout whose
// prefix pair is negative, decreasing or ends beyond det_rows is empty (and its list is not read).
struct DetFrame { long long r0, n; const int* kl; int k; };
__device__ static inline DetFrame det_frame(const int* keep, const int* prefix, int b, int slots, long long det_rows) {
    DetFrame f;
    if (prefix) {
        const long long p0 = prefix[b], p1 = prefix[b + 1];
        const bool ok = p0 >= 0 && p1 >= p0 && p1 <= det_rows;
        f.r0 = ok ? p0 : 0;
        f.n = ok ? p1 - p0 : 0;
        f.kl = keep + (ok ? p0 + b : 0);
    } else {
        f.r0 = (long long)b * slots;
        f.n = slots;
        f.kl = keep + (long long)b * (slots + 1);
    }
    const long long lim = f.n < slots ? f.n : slots;
    const int c = lim > 0 ? f.kl[0] : 0;
    f.k = c < 0 ? 0 : (c > lim ? (int)lim : c);
    return f;
}

// The host-side requirements on the description, for entry point `fn` whose kernel holds at most max_slots list positions per frame.
static int det_rows_check(const char* fn, int32_t det_cols, int64_t det_rows, const int32_t* prefix, int32_t batch, int32_t slots,
                          int32_t max_slots) {
    DBX_REQUIRE(batch >= 0, "%s: batch=%d is negative", fn, batch);
    DBX_REQUIRE(det_cols == 5 || det_cols == 13, "%s: det_cols=%d must be 5 or 13", fn, det_cols);
    DBX_REQUIRE(slots >= 1 && slots <= max_slots, "%s: slots=%d must be 1..%d", fn, slots, max_slots);
    DBX_REQUIRE(det_rows >= 0, "%s: det_rows=%lld is negative", fn, (long long)det_rows);
    DBX_REQUIRE(prefix || det_rows >= (int64_t)batch * slots, "%s: det_rows=%lld is below batch * slots = %lld", fn, (long long)det_rows,
                (long long)batch * slots);
    return DBX_OK;
}
