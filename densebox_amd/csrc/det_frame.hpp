// The reading rule of a batch of detections as the decodes leave them on the device, shared by every kernel behind them that walks the
// kept rows (track_ops.hip, viz_ops.hip).
#pragma once

// Where frame b's rows and keep list are, from device data that is never trusted as a bound (the description dbx_match_gt_batch takes,
// eval_ops.hip): r0 the frame's first row of dets, n its rows, kl its keep list (the count, then row numbers within the frame), k the
// clamped count.  A frame of the packed layout whose prefix pair is negative, decreasing or ends beyond det_rows is empty.
struct TrackFrame { long long r0, n; const int* kl; int k; };
__device__ static inline TrackFrame track_frame(const int* keep, const int* prefix, int b, int slots, long long det_rows) {
    TrackFrame f;
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
