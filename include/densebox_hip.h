/*
 * densebox_hip.h -- C ABI of libdensebox_hip.so (MI355X / gfx950 only).
 *
 * The reference (CaptainEven/DenseBox) has NO native/FFI interface: its only
 * boundary is the Python surface of DenseBox.py.  This header is
 * therefore the boundary the build defines for the hot path; each entry point
 * names the reference lines whose arithmetic it replaces.  The Python front end
 * (densebox_amd/) binds these with ctypes.
 *
 * Conventions
 *  - every function returns 0 on success, a negative dbx_status otherwise, and
 *    never throws across the ABI; dbx_last_error() gives a thread-local message.
 *  - all pointers are DEVICE pointers owned by the caller (torch allocates);
 *    the library owns nothing, keeps no state between calls, and is re-entrant.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *    every call is asynchronous with respect to the host.
 *  - activations are "framed NHWC": [N][H+2p][W+2p][ld] elements of the compute
 *    dtype, the p-pixel frame is zero and is never written by any kernel.
 */
#ifndef DENSEBOX_HIP_H
#define DENSEBOX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum dbx_status {
    DBX_OK = 0,
    DBX_ERR_ARG = -1,      /* bad descriptor / unsupported shape */
    DBX_ERR_HIP = -2,      /* a HIP runtime call failed (launch, memset) */
    DBX_ERR_DTYPE = -3
};

enum dbx_dtype { DBX_F16 = 0, DBX_BF16 = 1, DBX_F32 = 2 };

const char* dbx_last_error(void);
/* ABI version of the header a caller was compiled against; dbx_version() returns the library's.  Bumped whenever a struct layout,
 * an argument list or a scratch-size contract changes (a binding must refuse a library whose version differs):
 *   2  (round 3) dbx_loss_forward_backward's scratch grew from n doubles to dbx_loss_scratch_bytes(n) (mask planes + partial sums);
 *      the dbx_pack_multi job record's former pad field became rows_lim
 *   3  (round 4) fused entry points added (see the round-4 section below); nothing removed
 *   4  (round 4) dbx_head2_backward_up takes a d_hid view with a NULL ptr ("do not store it"); heads-gen entry points added
 *   5  (round 4) dbx_sgd_pack_step and dbx_heads_forward_fused_heads added; nothing changed
 *   6  (round 5) dbx_conv_plan may name DBX_K_P8 (the 8-phase kernel: plain packed weights); dbx_heads_forward_fusable returns WHICH kernel
 *      takes the fused heads forward (1 = ws / fragment-order weights as before, 2 = 8-phase / plain weights + plain second-weight image)
 *   7  (round 6) additions only: dbx_grad_guard, dbx_sgd_step_guarded, dbx_sgd_pack_step_guarded (f16 overflow guard), dbx_conv_wgrad_pool_dz; the heads-gen
 *      entry points accept DBX_F32 (reference instantiations for the parity suite)
 *   8  additions only: dbx_detect_batch, dbx_detect_batch_scratch_bytes (one decode + NMS launch over a batch of images)
 *   9  additions only: dbx_warp_job, dbx_warp_perspective_batch_u8, dbx_warp_batch_workspace_bytes (every plate of a batch in one launch)
 *  10  additions only: dbx_resize_job, dbx_resize_cubic_batch_u8, dbx_resize_batch_workspace_bytes (batched pad + bicubic resize)
 *  11  additions only: dbx_merge_xform, dbx_merge_nms_batch, dbx_merge_nms_batch_workspace_bytes (pyramid levels merged + one NMS per frame)
 *  12  additions only: dbx_detect_thresh_batch, dbx_detect_thresh_batch_scratch_bytes (score-threshold decode, packed results),
 *      dbx_nms_large, dbx_nms_large_scratch_bytes (greedy NMS for up to 4096 rows on many CUs)
 *  13  additions only: dbx_thresh_rows_batch, dbx_thresh_rows_batch_scratch_bytes (the threshold decode's rows without its NMS),
 *      dbx_merge_nms_thresh_batch, dbx_merge_nms_thresh_batch_workspace_bytes (pyramid merge + NMS over per-level row counts that
 *      stay on the device)
 *      also at 13, without a bump: dbx_crop_frame, dbx_plate_crops_batch (fixed-size plate crops rectified on the device).  A pure
 *      addition changes no layout, argument list or scratch contract, so a binding written against 13 stays valid; a binding that needs
 *      the new entry point looks the symbol up
 *      also at 13, without a bump: dbx_eval_record, dbx_match_gt_batch, dbx_eval_append (detections matched to ground truth and the
 *      records of an evaluation pass accumulated on the device), pure additions likewise
 *      also at 13, without a bump: dbx_track, dbx_track_record, dbx_track_update_batch, dbx_track_append (multi-stream tracking by
 *      detection with its state on the device), pure additions likewise
 *      also at 13, without a bump: dbx_shot, dbx_shot_record, dbx_crop_sharpness, dbx_track_gallery_update (the best plate crop of
 *      every track kept on the device), pure additions likewise
 *      also at 13, without a bump: dbx_overlay_frame, dbx_overlay_style, dbx_draw_overlay_batch, dbx_overlay_font, dbx_overlay_label
 *      (annotated frames painted on the device), pure additions likewise
 *      also at 13, without a bump: dbx_patch_job, dbx_patch_geom, dbx_patch_plan_io, dbx_patch_plan, dbx_patch_cut, dbx_patch_plan_host,
 *      dbx_patch_draw, dbx_patch_check_tables (training patches sampled and cut on the device), pure additions likewise
 *      also at 13, without a bump: dbx_head2_up_plan_t, dbx_head2_backward_up_plan (which launches dbx_head2_backward_up makes: a
 *      read-only host query), a pure addition likewise
 *      also at 13, without a bump: dbx_upsample_bwd_plan_t, dbx_upsample_bilinear_bwd_plan (which kernel dbx_upsample_bilinear_bwd
 *      launches: a read-only host query), a pure addition likewise
 *      also at 13, without a bump: dbx_patch_warp_rec, dbx_patch_warp_cfg, dbx_patch_warp_io, dbx_patch_warp_plan, dbx_patch_warp,
 *      dbx_patch_warp_params_host, dbx_patch_warp_host (training patches warped on the device), pure additions likewise
 *      also at 13, without a bump: dbx_redact_style, dbx_redact_batch, dbx_redact_host (plates made unreadable on the device), pure
 *      additions likewise
 *      also at 13, without a bump: dbx_nv12_frame, dbx_nv12_params, dbx_resize_job_nv12, dbx_nv12_to_rgb_batch, dbx_rgb_to_nv12_batch,
 *      dbx_nv12_host, dbx_resize_batch_nv12_workspace_bytes, dbx_resize_cubic_batch_nv12 (NV12 frames converted to and from RGB and
 *      resized straight from the surface), pure additions likewise
 *      also at 13, without a bump: dbx_zone_line, dbx_zone_poly, dbx_zone_config, dbx_zone_state, dbx_zone_event, dbx_zone_filter_keep,
 *      dbx_zone_update_batch, dbx_zone_append, dbx_zone_check_config, dbx_zone_host (region-of-interest filter, line crossings and
 *      region events behind the tracker), pure additions likewise
 *      also at 13, without a bump: dbx_tile, dbx_tile_grid, dbx_tile_stage_bytes, dbx_tile_rows_batch,
 *      dbx_tile_nms_batch_workspace_bytes, dbx_tile_nms_batch, dbx_tile_host (tiled detection: the plan of a large frame and the
 *      per-frame stitch of the tiles' rows on the device), pure additions likewise */
#define DBX_ABI_VERSION 13
int dbx_version(void);
/* device sanity: returns gfx arch number (950) of `device`, or <0 */
int dbx_device_arch(int device);

/* ------------------------------------------------------------------ framed NHWC tensor view */
typedef struct dbx_view {
    void*   ptr;      /* element (n=0, y=-pad, x=-pad, c=0) of the frame */
    int32_t n, h, w;  /* logical (unframed) extent */
    int32_t pad;      /* frame width in pixels (0, 1, or kh-1 for the un-padded refine convs' gradients) */
    int32_t ld;       /* elements per pixel (>= c_off + c) */
    int32_t c_off;    /* first channel this view addresses */
    int32_t c;        /* channels in this view */
} dbx_view;

/* ------------------------------------------------------------------ convolution (implicit GEMM on MFMA)
 * y[n,oy,ox,co] = epi( sum_{ky,kx,ci} x[n, oy+ky-cpad, ox+kx-cpad, ci] * w[co][ky][kx][ci] + bias[co] )
 * Replaces nn.Conv2d(+ReLU) at DenseBox.py:185-209 (3x3 backbone), :223-224/:455-461/:717-726
 * (1x1 heads), :466-471 (refine branch), and -- with transposed/flipped packed weights --
 * autograd's dgrad of the same layers (DenseBox.py:2186 loss.backward()).
 */
enum dbx_epilogue {
    DBX_EPI_BIAS     = 1,   /* + bias[co] (fp32) */
    DBX_EPI_RELU     = 2,   /* max(.,0) */
    DBX_EPI_GATE     = 4,   /* zero where gate[n,oy,ox,co] <= 0 (ReLU backward; gate = forward activation) */
    DBX_EPI_DROPMASK = 8,   /* * 2 * mask[m][co] (uint8 {0,1}, unframed [M][c]) -- nn.Dropout(0.5) with a caller-supplied mask */
    DBX_EPI_ACCUM    = 16,  /* y += result (dtype of y) */
    DBX_EPI_F32_NCHW = 32,  /* write fp32 NCHW [N][cv][Ho][Wo] (cv = y->c valid channels) instead of framed NHWC */
    DBX_EPI_DROPHASH = 64,  /* nn.Dropout(0.5) with the keep bit of element (m, co) = dbx_drop_keep(desc.drop_seed, m, co): no mask
                               buffer; dbx_head2_dgrad regenerates the same bits in backward */
    DBX_CONV_WFRAG   = 128  /* not an epilogue: w_packed is in MFMA-fragment order (dbx_pack_weight modes 4/5), the layout
                               dbx_conv_plan() asks for when it selects the register-streamed-weights kernel */
};

typedef struct dbx_conv_desc {
    int32_t dtype;         /* dbx_dtype of x, w and (unless F32_NCHW) y */
    int32_t kh, kw;        /* 1x1, 3x3, 5x5 */
    int32_t cpad;          /* conv padding (0 or 1); x->pad >= cpad */
    int32_t cin_pad;       /* channels per tap in the packed weight (multiple of 16 bytes worth) */
    int32_t cout_pad;      /* rows of the packed weight (multiple of 64) */
    int32_t epilogue;      /* OR of dbx_epilogue */
    uint32_t drop_seed;    /* DBX_EPI_DROPHASH: per-step seed of the counter-based keep mask */
} dbx_conv_desc;

/* packed weight: [cout_pad][ktot] elements, ktot = roundup(kh*kw*cin_pad*esize, 128 B)/esize, k = tap*cin_pad + ci */
int64_t dbx_conv_packed_elems(const dbx_conv_desc* d);
int dbx_conv_forward(const dbx_conv_desc* d, const dbx_view* x, const void* w_packed, const float* bias,
                     const dbx_view* y, const dbx_view* gate, const uint8_t* dropmask, int32_t dropmask_ld,
                     void* stream);
/* Which kernel dbx_conv_forward would run for (d, x, y), and the weight layout it wants.  The caller packs the weights
 * accordingly (w_frag != 0: dbx_pack_weight mode 4 (forward) / 5 (dgrad) and DBX_CONV_WFRAG in d->epilogue; else modes 0 / 1).
 * `name` is the kernel family and tile as it appears in a rocprofv3 trace (bench.py labels its roofline with it). */
enum dbx_conv_kernel { DBX_K_IGEMM = 1, DBX_K_DMA = 2, DBX_K_BAND = 3, DBX_K_C64 = 4, DBX_K_C8 = 5, DBX_K_WS = 6, DBX_K_P8 = 7 };
typedef struct dbx_conv_plan_t {
    int32_t kernel;        /* dbx_conv_kernel */
    int32_t tile_m, tile_n;
    int32_t w_frag;        /* 1: fragment-order weights wanted */
    char    name[64];
} dbx_conv_plan_t;
int dbx_conv_plan(const dbx_conv_desc* d, const dbx_view* x, const dbx_view* y, dbx_conv_plan_t* out);

/* Heads forward, BOTH 1x1 convs of every head in one pass over the pixels (DenseBox.py:158-162 x nh heads; round 4):
 *   hid = Dropout(Conv1x1(768 -> 512)(x))  for the nh heads side by side (d: 1x1, cin_pad 768, cout_pad 512 nh, epilogue
 *   DBX_EPI_BIAS | DBX_EPI_DROPHASH | DBX_CONV_WFRAG, w1_frag = dbx_pack_weight mode 4) -- written to `hid` as dbx_conv_forward would,
 *   out[n][off_i + m][y][x] = bias2[off_i + m] + sum_c W2_i[m][c] hid[n][y][x][512 i + c]   (fp32 NCHW, [N][sum k][H][W]; off_i = k_0 + .. + k_{i-1})
 * from the tile while it is in registers (the rounded, dropped values that land in `hid`; fp32 accumulation; fixed summation order).
 * w2_frag: the nh second weights as ONE dbx_pack_weight mode-4 image of 256 rows x (512 nh) columns, head i's k_i rows at rows
 * 0..k_i-1 (row_off 0) and columns 512 i.. (k_off 512 i).  scratch: dbx_heads_forward_fused_scratch_bytes(nh, N H W).
 * dbx_heads_forward_fusable() names the kernel that takes the call (16-bit types, k_i <= 8), 0 = none (run dbx_conv_forward twice):
 *   1 = the 1x1 register-streamed-weights kernel: d->epilogue carries DBX_CONV_WFRAG, w1_frag / w2_frag are the mode-4 images above;
 *   2 = the 8-phase kernel (round 5; ABI version 6): NO DBX_CONV_WFRAG, w1_frag = the plain dbx_pack_weight mode-0 image [512 nh][768],
 *       w2_frag = ONE plain mode-0 image of 64 rows x (512 nh) columns, head i's k_i rows at rows 0..k_i-1 (row_off 0) and columns 512 i..
 *       (k_off 512 i), zero elsewhere.  Same scratch, same outputs, same dropout masks (dbx_drop_hash32 of seed, pixel, channel / 32).
 * A caller that passes DBX_CONV_WFRAG always gets the ws kernel where that one can run the problem. */
int dbx_heads_forward_fusable(const dbx_conv_desc* d, const dbx_view* x, const dbx_view* hid, const int32_t* k, int32_t nh);
int64_t dbx_heads_forward_fused_scratch_bytes(int32_t nh, int64_t pixels);
int dbx_heads_forward_fused(const dbx_conv_desc* d, const dbx_view* x, const void* w1_frag, const float* bias1, const dbx_view* hid,
                            const void* w2_frag, const float* bias2, const int32_t* k, int32_t nh, float* out_nchw, void* scratch,
                            void* stream);
/* The same with one destination per head, as the reference's forward returns them (DenseBox.py:223-224): outs[i] = head i's own
 * contiguous fp32 [N][k_i][H][W] tensor (host array of nh device pointers).  Saves the caller the nh slice copies out of [N][sum k][H][W]. */
int dbx_heads_forward_fused_heads(const dbx_conv_desc* d, const dbx_view* x, const void* w1_frag, const float* bias1, const dbx_view* hid,
                                  const void* w2_frag, const float* bias2, const int32_t* k, int32_t nh, float* const* outs, void* scratch,
                                  void* stream);

/* 1x1 GEMM (16-bit types) with a split destination: couts [0, split_c) go to y with d->epilogue / gate, couts
 * [split_c, split_c + y2->c) to y2 with epilogue2 (plain, GATE and/or ACCUM) / gate2.  split_c = y->c, a multiple of 256.
 * Used for the data gradient of the fusion concat (torch.cat, DenseBox.py:219): one pass over the 2048-channel hidden
 * gradient feeds both the up-sampled conv4_4 branch and the conv3_4 branch. */
int dbx_conv_forward_split(const dbx_conv_desc* d, const dbx_view* x, const void* w_packed, const float* bias,
                           const dbx_view* y, const dbx_view* gate, const dbx_view* y2, const dbx_view* gate2,
                           int32_t split_c, int32_t epilogue2, void* stream);

/* dbx_conv_forward with the 2x2 / stride 2 max pooling of its output done in the epilogue (conv1_2 -> pool1,
 * DenseBox.py:186-187): `ypool` (N x H/2 x W/2 x 64) receives exactly what dbx_maxpool2x2 would make of y; with
 * write_full == 0 only the pooled map is written (inference: nothing re-reads the full-resolution map).  Exists for the
 * problems dbx_conv_pool_fusable() returns 1 for -- 16-bit 3x3 / pad 1 on congruent frames, even H and W: 64 -> 64 channels with an
 * epilogue within BIAS | RELU (the halo-tile kernel), or a layer the 8-phase kernels take (DBX_K_P8: conv2_2 -> pool2, conv3_4 ->
 * pool3, DenseBox.py:191, :204) with a (BIAS |) RELU epilogue, `ypool` N x H/2 x W/2 x y->c; anything else is DBX_ERR_ARG and the
 * caller runs the two calls.  dbx_conv_pool_fusable() answers for (d, x, y) only: a 1 holds for every `ypool` that is a frame of exactly
 * N x H/2 x W/2 pixels with c == y->c channels whose base, ld and c_off are multiples of 16 bytes (any pad >= 0) -- the call checks those
 * on the real view (DBX_ERR_ARG otherwise) -- and a 0 leaves dbx_last_error() as it was. */
int dbx_conv_pool_fusable(const dbx_conv_desc* d, const dbx_view* x, const dbx_view* y);
int dbx_conv_forward_pool(const dbx_conv_desc* d, const dbx_view* x, const void* w_packed, const float* bias,
                          const dbx_view* y, const dbx_view* ypool, int32_t write_full, void* stream);
/* ... and the arg-max nibbles of the pooled map in `idx` (layout of dbx_maxpool2x2_idx; null: not written).  With them a training
 * step needs the full-resolution conv1_2 output for nothing -- its only other reader was the pooling backward -- so write_full = 0
 * saves the 472 MB store (batch 64) and dbx_maxpool2x2_bwd_idx the 472 MB re-read.  With a ReLU epilogue (conv1_2) the nibbles are
 * bitwise those dbx_maxpool2x2_idx takes from the full map (window logic on the rounded values); without one they are taken from
 * the fp32 values before rounding (two window elements that round to the same number: the one the fp32 computation picks). */
int dbx_conv_forward_pool_idx(const dbx_conv_desc* d, const dbx_view* x, const void* w_packed, const float* bias,
                              const dbx_view* y, const dbx_view* ypool, int32_t write_full, void* idx, void* stream);

/* fp32 OIHW [co][ci][kh][kw] -> packed compute-dtype weight.
 * mode 0: forward            wp[co][tap][ci]            = w[co][ci][tap]
 * mode 1: dgrad (transposed) wp[ci][taps-1-tap][co]     = w[co][ci][tap]   (rows = ci, "cin" = co)
 * mode 4 / 5: the same two matrices in MFMA-fragment order for the register-streamed-weights 3x3 kernel (rows_pad a
 *   multiple of 128, cin_pad of 64): element (row, tap = 3 ky + kx, k) at
 *   [row / BN][3 * (k / 64) + ky][kx * 4 + (k % 64) / 16][(row % BN) / 32][32 * ((k % 16) / 8) + row % 32][k % 8],
 *   BN = 256 if rows_pad % 256 == 0 else 128, KC = cin_pad / 64 -- one 1-KiB block is the A operand of one
 *   v_mfma_f32_32x32x16 for all 64 lanes.  Same size as modes 0 / 1.
 * row_off / k_off place the tensor inside a larger packed matrix (several heads' 1x1 weights side by side); elements whose
 * destination row / column falls outside [0, rows_pad) x [0, cin_pad) are skipped, so a NEGATIVE offset packs a channel range of
 * a wider tensor (the conv4_4 / conv3_4 parts of the 768-channel head weights). */
int dbx_pack_weight(int32_t dtype, int32_t mode, const float* w_oihw, int32_t co, int32_t ci, int32_t kh, int32_t kw,
                    void* w_packed, int32_t rows_pad, int32_t cin_pad, int32_t row_off, int32_t k_off, void* stream);

/* All parameters in ONE launch (after an optimizer step).  `jobs` is a device array of
 *   struct { const float* src; void* dst; int32 co, ci, taps, mode; int64 ktot; int32 cin_pad, row_off, k_off; }
 * followed by int32 rows_lim (rows of dst for modes 0/1, 0 = unchecked; the record is 56 bytes).
 * mode 0/1/4/5 as dbx_pack_weight (4/5: ktot carries rows_pad; out-of-range destinations are skipped), mode 2 = fp32 bias copy
 * into dst[row_off ...] (co = length, ci = taps = 1). */
int dbx_pack_multi(int32_t dtype, const void* jobs, int32_t count, int64_t max_elems, void* stream);

/* The optimizer step (dbx_sgd_step, below) AND the re-packing in one launch (round 4): one job per parameter updates it -- the bits of
 * dbx_sgd_step -- while its tiles are staged and emits ALL of its packed images from them (the parameter, its gradient and its
 * momentum buffer are read once; replaces dbx_sgd_step + dbx_pack_multi after a training step).  `jobs` is a device array of 192-byte records
 *   struct { float* p; int32 pidx, co, ci, taps, ndst, tiled;
 *            struct { void* dst; int64 ktot; int32 mode, cin_pad, row_off, k_off, rows_lim, pad; } d[4]; }
 * p = the fp32 OIHW parameter; pidx = its index in `ptrs` (the table dbx_sgd_step takes: [param, grad, momentum] x count; pidx < 0:
 * no gradient this step, the job only re-packs); d[0 .. ndst) = its destinations, fields as in dbx_pack_multi's record (ndst = 0: plain
 * update); tiled = 1 where every destination is a 16-bit image with 8-aligned offsets / paddings, its K index over a multiple of 8 source
 * channels and taps <= 25 (the staged-tile path; 0 = element-wise).  max_elems = the largest co ci taps. */
int dbx_sgd_pack_step(int32_t dtype, const void* jobs, int32_t count, int64_t max_elems, float* const* ptrs, float lr, float momentum,
                      float weight_decay, int32_t first_step, void* stream);

/* heads: data gradient of the nh (<= 4) Conv1x1(512->k_h) layers behind Dropout in one rank-k streaming pass:
 * d_hid[m, 512h+c] = keep(m, 512h+c) * sum_{j<k_h} d_out[m, slot*h + j] * w2[h][j][c];  keep = 2*mask[..] (dropmask buffer),
 * 2*hash bit (use_hash, same bits as DBX_EPI_DROPHASH with drop_seed) or 1 (neither)
 * d_out: nh equal channel slots (>= 8 each); w2[h]: fp32 [k_h][512]; w2 / k are HOST arrays (DenseBox.py:158-162) */
int dbx_head2_dgrad(int32_t dtype, const dbx_view* d_out, const float* const* w2, const int32_t* k, int32_t nh,
                    const dbx_view* d_hid, const uint8_t* dropmask, int32_t dropmask_ld, int32_t use_hash, uint32_t drop_seed,
                    void* stream);
/* Weight/bias gradients of the same stage-2 head convs in one streaming pass over the hidden map:
 * dw[h] fp32 [k[h]][512] (OIHW of the 1x1 conv), db[h] fp32 [k[h]] (may be NULL).  scratch: dbx_head2_wgrad_scratch_bytes
 * (rows = N * H of the maps).  Replaces autograd's weight gradient of `nn.Conv2d(512, k, 1)` at DenseBox.py:161,168,
 * :458-461, :720-726. */
int64_t dbx_head2_wgrad_scratch_bytes(int32_t nh, int32_t rows);
int dbx_head2_wgrad(int32_t dtype, const dbx_view* d_out, const dbx_view* hid, const int32_t* k, int32_t nh,
                    float* const* dw, float* const* db, void* scratch, void* stream);
/* Both of the above in ONE pass over the pixels (the d_hid write overlaps the hid read); results are bitwise those of
 * dbx_head2_wgrad followed by dbx_head2_dgrad.  scratch as for dbx_head2_wgrad. */
int dbx_head2_backward(int32_t dtype, const dbx_view* d_out, const dbx_view* hid, const float* const* w2, const int32_t* k,
                       int32_t nh, const dbx_view* d_hid, const uint8_t* dropmask, int32_t dropmask_ld, int32_t use_hash,
                       uint32_t drop_seed, float* const* dw, float* const* db, void* scratch, void* stream);
/* The same plus d_g44 = up^T(d_hid), the transposed bilinear up-sampling (align_corners, DenseBox.py:446-449) of the hidden gradient
 * onto conv4_4's grid -- dbx_upsample_bilinear_bwd(d_hid, d_g44, no gate) -- in the same pass: the 2048-channel gradient is not read
 * back.  d_hid is bitwise dbx_head2_dgrad's and d_g44 bitwise dbx_upsample_bilinear_bwd's; dw/db are summed per image (fixed order).
 * 16-bit types run fused when d_hid is up to 64 and d_g44 up to 32 pixels wide (up-sampling by ~2); everything else runs the two passes. */
int dbx_head2_backward_up(int32_t dtype, const dbx_view* d_out, const dbx_view* hid, const float* const* w2, const int32_t* k,
                          int32_t nh, const dbx_view* d_hid, const uint8_t* dropmask, int32_t dropmask_ld, int32_t use_hash,
                          uint32_t drop_seed, float* const* dw, float* const* db, void* scratch, const dbx_view* d_g44, void* stream);
/* Round 6: a weight gradient whose dz is the backward of a 2x2 / stride 2 max pooling need not see that map in memory either:
 * dbx_conv_wgrad_pool_dz == dbx_maxpool2x2_bwd_idx(idx, dy, dz, accumulate 0, relu_gate 1) followed by dbx_conv_wgrad(dz, x, ...), bit for bit,
 * without dz (conv1_2's weight gradient behind pool1, DenseBox.py:186-187 backwards: 148 MB of dy + nibbles read instead of the 472 MB map).
 * dy: the pooled gradient (N x H/2 x W/2, same channels / channel offset as dz); idx: the arg-max nibbles of the WHOLE pooled layer
 * (dbx_maxpool2x2_idx layout, idx_channels channels per pooled pixel); dz: the shape of the un-pooled gradient on its frame (congruent with
 * x; ptr is not read -- unless write_dz != 0: then the kernel ALSO writes the un-pooled gradient map there, every pixel of the frame incl. its
 * zero halo, bit for bit dbx_maxpool2x2_bwd_idx's, for a consumer that still wants it in memory: the pooling backward's own launch goes
 * away).  Exists where dbx_conv_wgrad_pool_dz_ok() returns 1 (16-bit, even H / W, the 3x3 column-strip kernel's shapes, dz->c a
 * multiple of 64 inside its ld) and co == dz->c -- the kernel loads dy and the nibbles in whole 64-channel tiles; anything else is refused;
 * scratch as dbx_conv_wgrad_scratch_bytes(dz, x). */
int dbx_conv_wgrad_pool_dz_ok(int32_t dtype, const dbx_view* dz, const dbx_view* x, int32_t kh, int32_t kw);
int dbx_conv_wgrad_pool_dz(int32_t dtype, const dbx_view* dy, const void* idx, int32_t idx_channels, const dbx_view* dz, const dbx_view* x,
                           int32_t kh, int32_t kw, int32_t cpad, int32_t co, int32_t ci, float* dw_oihw, float* db, void* scratch,
                           int32_t accumulate, int32_t write_dz, void* stream);
/* Round 4: the hidden gradient need not exist in memory.  d_hid = keep * scale * (d_out W2) has <= 8 input channels per head, so
 * its consumers GENERATE it, 32 channels x 32 pixels per MFMA (W2 and d_out in the compute dtype, keep bits from the forward's hash):
 *   dbx_head2_backward_up with d_hid->ptr == NULL (the view's shape still describes the map) does not store it (one-pass form
 *     only: dbx_head2_backward_up_fused() == 1; hash dropout or none; it rounds W2 to the compute dtype like the generators),
 *   dbx_heads1_wgrad_gen = dbx_conv_wgrad_slice(d_hid, x, 1x1, ...) (x on a padded frame of >= 32 columns: dbx_heads1_wgrad_gen_ok();
 *     16-bit types: fewer than 2**24 pixels N H W in all -- the generator's 24-bit index multiply, the bound dbx_heads1_dgrad_gen has
 *     too; at or beyond it the call is refused and dbx_heads1_wgrad_gen_ok() is 0),
 *   dbx_heads1_dgrad_gen = dbx_conv_forward(d_hid, W1^T, DBX_EPI_GATE) -> y (256 channels; w1t_frag = dbx_pack_weight mode 5 image,
 *     rows_pad 256, cin_pad 512 nh).
 * d_out: the compact [N, H, W] map (pad 0) with one slot of >= 8 channels per head, channels >= k[i] zero; w2[i]: fp32 [k[i]][512].
 * Results equal the in-memory forms up to fp32 summation order (W2 representable in the compute dtype) / its rounding (otherwise).
 * DBX_F32 (round 6): plain one-thread-per-output reference instantiations of the two generators (csrc/heads_ref_f32.hip) so that the
 * exact-fp32 path can run the 16-bit step's call structure against the reference-captured gradients; there d_out slots may be any
 * width >= k, x / y / gate any frames, w1t_frag is the PLAIN dbx_pack_weight mode 1 image (rows of 512 nh floats) and scratch is unused.
 * (Heads: DenseBox.py:158-162, :174-178; their backward is autograd's in the reference.) */
int dbx_head2_backward_up_fused(int32_t dtype, const dbx_view* hid, const dbx_view* d_g44);
/* What dbx_head2_backward_up would run for (dtype, hid, d_g44, k[0 .. nh)): a read-only query on the host -- nothing is launched, no
 * view's ptr is followed -- computed by the helpers the entry point itself dispatches through (the tests of the stage-2 backward
 * assert from it which path a case takes).  fused 0: the two passes (dbx_head2_backward, then dbx_upsample_bilinear_bwd); every other
 * field is 0.  fused 1: `halves` workgroups share a row of the hidden map, half[i] walks its pixel columns [px_lo, px_lo + px_n),
 * stores and accumulates the columns [own_lo, own_hi) and reduces d_g44's columns [ix_lo, ix_lo + ix_n) (halves 1: half[1] repeats
 * half[0]); launch[0 .. launches) are the kernel launches in order: heads [head0, head0 + heads) with kj of their d_out channels
 * multiplied out (k rounded up to 1 / 2 / 4 / 8), `groups` workgroups per (64-channel slice, half) -- workgroup g walks the images g,
 * g + groups, ... -- and blocks = groups * halves partial weight-gradient blocks (the launch's grid is blocks * 8 * heads workgroups).
 * Layouts: dbx_head2_up_half 24 bytes (px_lo 0, px_n 4, own_lo 8, own_hi 12, ix_lo 16, ix_n 20); dbx_head2_up_launch 20 bytes (head0 0,
 * heads 4, kj 8, groups 12, blocks 16); dbx_head2_up_plan_t 140 bytes (fused 0, halves 4, half 8, launches 56, launch 60). */
typedef struct dbx_head2_up_half { int32_t px_lo, px_n, own_lo, own_hi, ix_lo, ix_n; } dbx_head2_up_half;
typedef struct dbx_head2_up_launch { int32_t head0, heads, kj, groups, blocks; } dbx_head2_up_launch;
typedef struct dbx_head2_up_plan_t {
    int32_t fused, halves;
    dbx_head2_up_half half[2];
    int32_t launches;
    dbx_head2_up_launch launch[4];
} dbx_head2_up_plan_t;
int dbx_head2_backward_up_plan(int32_t dtype, const dbx_view* hid, const dbx_view* d_g44, const int32_t* k, int32_t nh,
                               dbx_head2_up_plan_t* out);
int dbx_heads1_wgrad_gen_ok(int32_t dtype, const dbx_view* x, int32_t nh);
int dbx_heads1_wgrad_gen(int32_t dtype, const dbx_view* d_out, const dbx_view* x, const float* const* w2, const int32_t* k, int32_t nh,
                         int32_t use_hash, uint32_t drop_seed, int32_t ci, float* dw_oihw, int32_t dw_ci_total, int32_t dw_ci_off,
                         float* db, void* scratch, void* stream);
int dbx_heads1_dgrad_gen(int32_t dtype, const dbx_view* d_out, const float* const* w2, const int32_t* k, int32_t nh, int32_t use_hash,
                         uint32_t drop_seed, const void* w1t_frag, const dbx_view* y, const dbx_view* gate, void* stream);

/* eval-mode folding of one head, Conv1x1(768->512) -> Dropout(identity) -> Conv1x1(512->k), into a single 768->k map
 * (no non-linearity in between, DenseBox.py:158-162): w_out[k][768] = w2 w1, b_out[k] = w2 b1 + b2 (all fp32) */
int dbx_fold_heads(const float* w2, const float* b2, const float* w1, const float* b1, int32_t k, float* w_out,
                   float* b_out, void* stream);
/* Eval mode, refine branch (pool4 -> conv6_1 3x3 -> conv6_2 5x5 -> bilinear up -> conv6_3 1x1, DenseBox.py:464-471 / :729-736): nothing
 * after the pooling is non-linear, so the three convs fold into ONE un-padded 7x7 conv ci -> 1 (w_out [1][ci][7][7], b_out [1]) whose
 * single map is then up-sampled (dbx_upsample_bilinear_nchw_f32: fp32 NCHW planes, align_corners=True, ATen's arithmetic).  w1
 * [cm][ci][3][3], b1 [cm], w2 [cm][cm][5][5], b2 [cm], w3 [1][cm][1][1], b3 [1]; cm <= 64.  v_out [cm][5][5] = sum_n w3[n] w2[n][m] (the
 * 64 -> 1 fold of conv6_3 into conv6_2, which dbx_refine_backward needs as well). */
int dbx_fold_refine(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                    int32_t ci, int32_t cm, float* w_out, float* b_out, float* v_out, void* stream);
/* ... and the folded branch itself in one fp32 kernel: cat(landmarks [n][4][h][w], score [n][1][h][w]) (fp32 NCHW, the heads' outputs) ->
 * MaxPool2d(2, 2) -> that 7x7 conv -> out_small [n][1][h/2 - 6][w/2 - 6]; dbx_upsample_bilinear_nchw_f32 then gives the refined score. */
int dbx_refine_eval(const float* landmark_nchw, const float* score_nchw, int32_t n, int32_t h, int32_t w, const float* w_fold,
                    const float* b_fold, float* out_small, void* stream);
int dbx_upsample_bilinear_nchw_f32(const float* x, int32_t planes, int32_t hi, int32_t wi, float* y, int32_t ho, int32_t wo,
                                   void* stream);
/* Training: the backward pass of the same branch by the same linear structure (csrc/refine_ops.hip has the algebra).  With g = the
 * transposed up-sampling of d_refine and G1 = the folded conv's weight gradient (245 numbers + sum g), every parameter gradient of
 * conv6_1 / conv6_2 / conv6_3 is a small contraction of G1 with the weights, and the gradient of cat(landmarks, score) is the
 * transposed folded conv of g routed through the pooling arg-max.  d_refine [n][1][h][w]; landmark [n][4][h][w] / score [n][1][h][w] =
 * the heads' fp32 NCHW outputs of the forward pass; w_fold / v_fold from dbx_fold_refine; g_landmark / g_score = the incoming gradients of
 * those two heads (null = zero), out_landmark / out_score = incoming + the branch's contribution; dw* / db* in the parameters' own
 * layouts (fp32, overwritten); scratch of dbx_refine_backward_scratch_bytes(n, h, w).  All sums in a fixed order (bitwise repeatable).
 * Reference: loss.backward() through DenseBox.py:464-471 (:2186 / :2731). */
int64_t dbx_refine_backward_scratch_bytes(int32_t n, int32_t h, int32_t w);
int dbx_refine_backward(const float* d_refine, const float* landmark, const float* score, int32_t n, int32_t h, int32_t w,
                        const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                        int32_t cm, const float* w_fold, const float* v_fold, const float* g_landmark, const float* g_score, float* out_landmark,
                        float* out_score, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* scratch,
                        void* stream);

/* ------------------------------------------------------------------ weight gradient
 * dw[co][ci][ky][kx] (+)= sum_{n,y,x} dz[n,y,x,co] * x[n,y+ky-cpad,x+kx-cpad,ci]   (fp32 OIHW, DenseBox.py:2186)
 * db[co] = sum dz.   dz and x must live in frames of identical geometry (same n,h,w,pad).
 * `partial` is a scratch buffer of dbx_conv_wgrad_scratch_bytes(); the reduction over it is deterministic.
 */
int64_t dbx_conv_wgrad_scratch_bytes(int32_t dtype, const dbx_view* dz, const dbx_view* x, int32_t kh, int32_t kw);
/* co/ci: real channel counts of dw_oihw [co][ci][kh][kw] (the views may be wider: padded channels are dropped).
 * db may be NULL.  accumulate != 0 adds into dw/db instead of overwriting. */
int dbx_conv_wgrad(int32_t dtype, const dbx_view* dz, const dbx_view* x, int32_t kh, int32_t kw, int32_t cpad,
                   int32_t co, int32_t ci, float* dw_oihw, float* db, void* scratch, int32_t accumulate, void* stream);
/* The same with dw a column slice of a wider tensor: dw_oihw is [co][dw_ci_total][kh][kw] and the ci input channels of x go to
 * columns [dw_ci_off, dw_ci_off + ci) -- the gradient of a convolution over a channel concat (torch.cat, DenseBox.py:219),
 * computed per concatenated tensor (the two may then live on different grids: see dbx_upsample_bilinear_bwd). */
int dbx_conv_wgrad_slice(int32_t dtype, const dbx_view* dz, const dbx_view* x, int32_t kh, int32_t kw, int32_t cpad,
                         int32_t co, int32_t ci, float* dw_oihw, int32_t dw_ci_total, int32_t dw_ci_off, float* db, void* scratch,
                         int32_t accumulate, void* stream);
/* The kernel dbx_conv_wgrad runs for this problem ("wgrad_row3_kernel<bf16>" ...) and its split-K factor: the library's own
 * selection, for profile labels (no caller-side copy of the rule).  name_len >= 32. */
int dbx_conv_wgrad_plan(int32_t dtype, const dbx_view* dz, const dbx_view* x, int32_t kh, int32_t kw, char* name, int32_t name_len,
                        int32_t* splits);

/* conv1_2's data gradient with conv1_1's weight/bias gradient folded into its epilogue (DenseBox.py:185-186 backwards):
 * d = conv_transpose(dz, w) * (gate > 0) is the dz operand of the first layer's weight gradient and of nothing else, so it is
 * contracted against the 8-channel framed network input x0 inside the kernel and never written:
 *   dw[co][c][tap] (+)= sum_px d[px][co] * x0[px + tap][c]  (c < ci <= 8),  db[co] (+)= sum_px d[px][co]
 * -- what dbx_conv_forward(GATE) into a d map followed by dbx_conv_wgrad(d, x0) produce, up to fp32 summation order.
 * d: the dgrad descriptor (3x3, cpad 1, 64 -> 64, epilogue DBX_EPI_GATE, weights packed with mode 1); exists where
 * dbx_conv_dgrad_wgrad1_fusable() returns 1.  scratch: dbx_conv_dgrad_wgrad1_scratch_bytes(). */
int64_t dbx_conv_dgrad_wgrad1_scratch_bytes(void);
int dbx_conv_dgrad_wgrad1_fusable(const dbx_conv_desc* d, const dbx_view* dz, const dbx_view* gate, const dbx_view* x0);
int dbx_conv_dgrad_wgrad1(const dbx_conv_desc* d, const dbx_view* dz, const void* w_packed, const dbx_view* gate, const dbx_view* x0,
                          int32_t ci, float* dw_oihw, float* db, void* scratch, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------ layout / pooling / resampling
 * nchw_to_framed: network input X (DenseBox.py:185) fp32 NCHW -> framed NHWC compute dtype (channels padded with 0).
 * maxpool2x2:     nn.MaxPool2d(2,2) floor mode (DenseBox.py:187,191,204,465), first-max-wins like ATen.
 * maxpool2x2_bwd: gradient routed to the arg-max, times ReLU gate of the pre-pool activation.
 * upsample:       nn.Upsample(size, bilinear, align_corners=True) (DenseBox.py:213-216, :468-470).
 */
/* x_nchw has c_src channels; channels c_src..y->c-1 of the framed view are written as 0 (also used for dL/dout) */
int dbx_nchw_to_framed(int32_t dtype, const float* x_nchw, int32_t c_src, const dbx_view* y, void* stream);
/* uint8 [N][H][W][3] images -> framed network input: ((u8/255) - mean[c]) / std[c] (fp32, true divisions), i.e. torchvision
 * ToTensor + Normalize of the reference datasets (DenseBox.py:766-772) fused with the layout change.  mean3/std3: HOST floats */
int dbx_u8hwc_to_framed(int32_t dtype, const uint8_t* x_nhwc, const dbx_view* y, const float* mean3, const float* std3,
                        void* stream);
/* scatter c_src fp32 NCHW planes into channels [c_dst_off, c_dst_off+c_src) of y; other channels untouched
 * (builds cat(landmarks, score), DenseBox.py:464 / :729) */
int dbx_nchw_to_framed_ch(int32_t dtype, const float* x_nchw, int32_t c_src, const dbx_view* y, int32_t c_dst_off,
                          void* stream);
/* nslots (<= 4) fp32 NCHW tensors x_nchw[i] (k[i] planes; a null pointer = zeros) into consecutive `slot`-channel ranges of ONE framed
 * view y (y->c == nslots * slot): channels k[i] .. slot-1 of a range are zeroed.  dL/d(head outputs) of all heads in one launch. */
int dbx_nchw_to_framed_slots(int32_t dtype, const float* const* x_nchw, const int32_t* k, int32_t nslots, int32_t slot,
                             const dbx_view* y, void* stream);
int dbx_framed_to_nchw_f32(int32_t dtype, const dbx_view* x, float* y_nchw, void* stream);
/* dst[..., c_dst_off+j] += src[..., c_src_off+j], j < n_ch (gradient of the channel concat at DenseBox.py:464) */
int dbx_framed_add_ch(int32_t dtype, const dbx_view* src, int32_t c_src_off, int32_t n_ch, const dbx_view* dst,
                      int32_t c_dst_off, void* stream);
int dbx_maxpool2x2(int32_t dtype, const dbx_view* x, const dbx_view* y, void* stream);
/* x = pre-pool activation, dy = grad of the pooled map, dx = grad of the pre-pool map (same frame as x) */
int dbx_maxpool2x2_bwd(int32_t dtype, const dbx_view* x, const dbx_view* dy, const dbx_view* dx,
                       int32_t accumulate, int32_t relu_gate, void* stream);
/* Training: the forward pooling also records WHERE each maximum came from, so that the backward pass reads the pooled gradient and
 * half a byte per pooled element instead of the whole un-pooled activation (nn.MaxPool2d backward, DenseBox.py:187 / :191 / :204
 * under loss.backward(), :2186).  idx: device buffer of dbx_maxpool_idx_bytes(n, h, w, c) bytes (h, w, c of the UN-pooled map),
 * 4-byte aligned, dense [n][h/2][w/2][c/2]: one nibble per pooled element, channel c in byte c/2 (even channel = low nibble);
 * bits 0..1 = window position of the first maximum in (0,0),(0,1),(1,0),(1,1) order (ATen's tie rule), bit 2 = (maximum > 0).
 * dbx_maxpool2x2_bwd_idx gives exactly dbx_maxpool2x2_bwd's result for the map the nibbles were taken from; relu_gate uses bit 2. */
int64_t dbx_maxpool_idx_bytes(int32_t n, int32_t h, int32_t w, int32_t c);
int dbx_maxpool2x2_idx(int32_t dtype, const dbx_view* x, const dbx_view* y, void* idx, void* stream);
int dbx_maxpool2x2_bwd_idx(int32_t dtype, const void* idx, const dbx_view* dy, const dbx_view* dx,
                           int32_t accumulate, int32_t relu_gate, void* stream);
int dbx_upsample_bilinear(int32_t dtype, const dbx_view* x, const dbx_view* y, void* stream);
/* gate (optional): forward activation of dx's tensor; dx is zeroed where gate <= 0 (ReLU backward) */
int dbx_upsample_bilinear_bwd(int32_t dtype, const dbx_view* dy, const dbx_view* dx, const dbx_view* gate, void* stream);
/* What dbx_upsample_bilinear_bwd would run for (dtype, dy, dx): a read-only query on the host -- nothing is launched, no view's ptr is
 * followed -- computed by the helper the entry point itself dispatches through (tests/test_hip_aux_paths.py asserts from it which
 * path a case takes).  kernel: 0 the flat gather (one lane per source pixel and 16-byte channel group: any geometry), 1 the tabulated
 * rows kernel (one workgroup per source row; both scales above 0.34 and dx at most 1536 wide), 2 the column walk (one workgroup per
 * pair of source rows and segment of source columns; both scales in (0.45, 1), at least 64 channel groups, dy at most 4096 wide and
 * its frame spanning fewer than 2^32 elements).  nseg: column segments per row pair (walk only, else 0); workgroups: the launch's
 * grid; lds_bytes: the dynamic LDS it asks for.  Layout: dbx_upsample_bwd_plan_t 16 bytes (kernel 0, nseg 4, workgroups 8,
 * lds_bytes 12). */
typedef struct dbx_upsample_bwd_plan_t { int32_t kernel, nseg, workgroups, lds_bytes; } dbx_upsample_bwd_plan_t;
int dbx_upsample_bilinear_bwd_plan(int32_t dtype, const dbx_view* dy, const dbx_view* dx, dbx_upsample_bwd_plan_t* out);

/* ------------------------------------------------------------------ dense per-pixel loss (DenseBox.py:2023-2180 etc.)
 * One call builds the label maps (a5-a8), element-wise L2, hard-negative mining (top-k per sample),
 * mask fill + gray zones (a11-a13), the weighted sums (a14/a15) and dL/d(out) for every head.
 */
typedef struct dbx_loss_desc {
    int32_t kind;            /* 0 DenseBox (train_online), 1 DenseBoxLM (train_LM_online), 2 DenseBoxLMLOC (train_densebox_online) */
    int32_t n;               /* local batch */
    int32_t half_neg;        /* hard negatives per sample = random negatives per sample (DenseBox.py:2081) */
    float   lambda_loc, lambda_det, lambda_lm;
    int32_t use_labels;      /* _pn variants: skip label==0 patches (kind 2) */
} dbx_loss_desc;

typedef struct dbx_loss_io {
    const float* bbox;       /* [n,4] 60-space corners */
    const float* vertices;   /* [n,8] or NULL */
    const float* labels;     /* [n,1] or NULL */
    const int64_t* rand_neg; /* [n,half_neg] */
    const int64_t* lm_rand_neg; /* [4,n,1] or NULL */
    const float* score;  const float* loc;  const float* lm;  const float* rf;  const float* lmloc;   /* fp32 NCHW outputs */
    float* d_score; float* d_loc; float* d_lm; float* d_rf; float* d_lmloc;                           /* fp32 NCHW grads (may be NULL) */
    float* loss;             /* [1] */
    float* mask_cls;         /* [n,1,60,60] out (debug/parity) or NULL */
    float* mask_lm;          /* [n,4,60,60] out or NULL */
    int64_t* neg_idx;        /* [n,2*half_neg] out or NULL */
    int64_t* lm_neg_idx;     /* [4,n,2] out or NULL */
    int32_t* pos_count;      /* [n] positives per sample out or NULL */
} dbx_loss_io;

/* scratch: dbx_loss_scratch_bytes(d->n) bytes, 8-byte aligned (per-workgroup partial sums, reduced in a fixed order, and the mask planes
 * the mining kernel hands to the gradient kernel) */
int64_t dbx_loss_scratch_bytes(int32_t n);
int dbx_loss_forward_backward(const dbx_loss_desc* d, const dbx_loss_io* io, void* scratch, void* stream);
/* positives per sample from the boxes alone (a5) -- lets the host derive half_neg without reading maps back */
int dbx_count_positives(const float* bbox, const float* labels, int32_t n, int32_t* count_per_sample, void* stream);

/* label-map generators as stand-alone ops (reference function names in DenseBox.py:1556-1914) */
int dbx_init_score_map(const float* bbox, const float* labels, int32_t n, float* out, void* stream);
int dbx_init_offset_map(const float* coords, const float* labels, int32_t n, int32_t c, float* out, void* stream);
int dbx_init_lm_heatmap(const float* vertices, const float* labels, int32_t n, int32_t clamp, float* out, void* stream);
int dbx_mask_by_sel(float* mask, int32_t n, const int64_t* pos_idx, int64_t n_pos, const int64_t* neg_idx, int32_t n_neg, void* stream);
int dbx_mask_gray_zone_cls(float* mask, const float* bbox, const float* labels, int32_t n, void* stream);
int dbx_mask_gray_zone_lm(float* mask, int32_t n, const int64_t* pos_idx, int64_t n_pos, void* stream);

/* ------------------------------------------------------------------ SGD (DenseBox.py:2001-2004, torch semantics)
 * for each tensor t: g = grad + wd*p; buf = first ? g : mu*buf + g; p -= lr*buf
 * ptrs: device array of 3*count pointers {p, grad, buf}; sizes: device array of count element counts.
 */
int dbx_sgd_step(float* const* ptrs, const int64_t* sizes, int32_t count, int64_t max_size,
                 float lr, float momentum, float weight_decay, int32_t first_step, void* stream);
/* Overflow guard of 16-bit training (round 6; no reference counterpart: the reference trains in fp32, DenseBox.py:2186-2187).  The f16 step
 * keeps dL/d(pre-activation) in f16 frames and the loss is an un-normalised sum (DenseBox.py:2917): a residual that overflows 65504 there
 * reaches every weight gradient behind it as inf / NaN.  dbx_grad_guard scans the step's gradients (one flat fp32 buffer, 16-byte aligned)
 * and leaves `step_id` (> 0, increasing from step to step) in guard[0] when any element is not finite; dbx_sgd_step_guarded /
 * dbx_sgd_pack_step_guarded launched with the same guard and step_id then change NOTHING (parameters, momentum buffers and packed images
 * stay as they were) and add 1 to guard[1], the count of skipped steps a caller reads back whenever it reads the loss.  guard: two
 * int32 on the device, zero-initialised by the caller; NULL = the unguarded update.  No host synchronisation anywhere. */
int dbx_grad_guard(const float* grads, int64_t n, int32_t* guard, int32_t step_id, void* stream);
int dbx_sgd_step_guarded(float* const* ptrs, const int64_t* sizes, int32_t count, int64_t max_size, float lr, float momentum,
                         float weight_decay, int32_t first_step, int32_t* guard, int32_t step_id, void* stream);
int dbx_sgd_pack_step_guarded(int32_t dtype, const void* jobs, int32_t count, int64_t max_elems, float* const* ptrs, float lr, float momentum,
                              float weight_decay, int32_t first_step, int32_t* guard, int32_t step_id, void* stream);

/* ------------------------------------------------------------------ decode + NMS (DenseBox.py:3114-3443)
 * top-K of the score map, corner/landmark decode to float64 rows [K, 5|13], greedy NMS (keep ovr <= thresh).
 * keep[0] = count, keep[1..] = kept row indices in reference order.
 */
int dbx_detect(const float* score, const float* loc, const float* lm_heat, const float* lm_loc,
               int32_t rows, int32_t cols, int32_t K, double nms_thresh,
               double* dets, int32_t det_cols, int64_t* topk_idx, int32_t* keep, void* scratch, void* stream);
int64_t dbx_detect_scratch_bytes(int32_t rows, int32_t cols, int32_t K);
/* the same over `batch` images in one launch (one workgroup per image): maps contiguous [batch][C][rows][cols] fp32 (C = 1, 4, 4, 8
 * for score, loc, lm_heat, lm_loc), dets [batch][K][det_cols], topk_idx [batch][K], keep [batch][K+1].  Image b's result is bit for
 * bit what dbx_detect gives on its own maps.  Scratch: dbx_detect_batch_scratch_bytes, one 256-byte-aligned slice per image of
 * dbx_detect_scratch_bytes rounded up to 256 bytes.  dbx_detect is this launch with batch = 1. */
int64_t dbx_detect_batch_scratch_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t K);
int dbx_detect_batch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc,
                     int32_t batch, int32_t rows, int32_t cols, int32_t K, double nms_thresh,
                     double* dets, int32_t det_cols, int64_t* topk_idx, int32_t* keep, void* scratch, void* stream);
/* scratch: 5*n bytes */
int dbx_nms(const double* dets, int32_t n, int32_t det_cols, double nms_thresh, int32_t* keep, void* scratch, void* stream);

/* ---- score-threshold decode (no reference counterpart as a function; per image it IS parse_*(maps, K = n_b) + NMS, DenseBox.py:3114-3443,
 * with n_b = min(#{score > score_thresh}, max_dets)): every pixel above the threshold becomes a row, the greedy NMS runs over all of
 * them.  Three launches on `stream` whose grids depend on (batch, max_dets) only; no host round trip, capturable.
 * Candidate set: score > score_thresh in fp32, strict -- a score equal to the threshold is out, NaN is never a candidate, +inf is,
 * -0.0 > 0.0 is false; score_thresh = -inf takes every number except -inf.  When more than max_dets (1..4096) pixels pass, the max_dets
 * best stay, in dbx_detect_batch's order: larger score first, the LOWER map index on ties (also for which of several equal scores
 * fall under the cap) -- exactly dbx_detect_batch with K = max_dets.  Rows are written in that order by the row writer dbx_detect_batch
 * uses; the NMS is dbx_nms's on them bit for bit (order: score descending, the HIGHER row first on ties; !(ovr <= thresh) suppresses).
 * Maps, det_cols and the lm_heat / lm_loc conventions are dbx_detect_batch's.  Outputs (device), P = counts' prefix:
 *   counts    int32 [batch][2] pairs (n_b, number of pixels above the threshold: > n_b when the cap cut), then int32 [batch + 1]:
 *             P[b] = n_0 + ... + n_(b-1), P[batch] = the number of rows of the call.  3 * batch + 1 words.
 *   dets      PACKED rows: image b's n_b rows of det_cols float64 start at row P[b].  Capacity batch * max_dets rows.
 *   topk_idx  packed likewise: the map index of every row.  Capacity batch * max_dets.
 *   keep      packed lists: image b's list is n_b + 1 words at word P[b] + b: the count, then the kept row numbers (0-based within the
 *             image) in the reference's order.  Capacity batch * (max_dets + 1).  Passing keep == (int32_t*)dets asks for the lists
 *             right BEHIND the packed rows, at byte P[batch] * det_cols * 8 of dets (capacity then batch * max_dets * det_cols * 8 +
 *             batch * (max_dets + 1) * 4 bytes): a host reads the counts, then rows and lists with one copy of
 *             P[batch] * (det_cols * 8 + 4) + batch * 4 bytes.
 * Nothing else of the outputs is written (an image without candidates writes its pair, its prefix word and a zero list count).
 * scratch: dbx_detect_thresh_batch_scratch_bytes(batch, rows, cols, max_dets) bytes (-1 for counts out of range), 256-byte-aligned
 * base, one slice per image (a multiple of 256 bytes: rows, indices, NMS order and the max_dets x ceil(max_dets / 64)-word suppression
 * matrix, 2 MB at 4096).  Refused with DBX_ERR_ARG before anything is launched: a null pointer (lm_heat / lm_loc excepted), batch < 1,
 * a bad map size, max_dets outside 1..4096, a NaN score_thresh, a NaN or negative nms_thresh, det_cols other than 5 or 13 with
 * landmark maps. */
int64_t dbx_detect_thresh_batch_scratch_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t max_dets);
int dbx_detect_thresh_batch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc,
                            int32_t batch, int32_t rows, int32_t cols, float score_thresh, int32_t max_dets, double nms_thresh,
                            double* dets, int32_t det_cols, int64_t* topk_idx, int32_t* keep, int32_t* counts, void* scratch,
                            void* stream);
/* The select stage of dbx_detect_thresh_batch alone -- one launch, no suppression matrix, no sweep, no keep list -- for a caller that
 * merges the rows of several runs before ONE NMS (dbx_merge_nms_thresh_batch).  Maps, score_thresh, max_dets, det_cols and the
 * refusals are dbx_detect_thresh_batch's.  Outputs (device), in SLOT layout:
 *   dets      [batch][max_dets][det_cols] float64: image b's n_b rows start at row b * max_dets; nothing beyond row n_b is written.
 *   topk_idx  [batch][max_dets] likewise.
 *   counts    int32 [batch][2]: (n_b, number of pixels above the threshold).
 * Rows and indices are bit for bit the first n_b rows dbx_detect_thresh_batch writes for the same inputs (one device function).
 * scratch: dbx_thresh_rows_batch_scratch_bytes(batch, rows, cols, max_dets) bytes (-1 for counts out of range), a non-null device
 * pointer; this version works in LDS and does not write it. */
int64_t dbx_thresh_rows_batch_scratch_bytes(int32_t batch, int32_t rows, int32_t cols, int32_t max_dets);
int dbx_thresh_rows_batch(const float* score, const float* loc, const float* lm_heat, const float* lm_loc,
                          int32_t batch, int32_t rows, int32_t cols, float score_thresh, int32_t max_dets,
                          double* dets, int32_t det_cols, int64_t* topk_idx, int32_t* counts, void* scratch, void* stream);
/* dbx_nms (DenseBox.py:3398-3443) for 1 <= n <= 4096 rows with the same keep list on every input (ties, NaN scores and boxes included):
 * a sort gives the order, the n x ceil(n / 64)-word suppression matrix is built by ceil(n / 64) workgroups, one wave walks it.
 * keep [n + 1]; scratch: dbx_nms_large_scratch_bytes(n) bytes (-1 outside 1..4096).  Refused: null pointers, n outside 1..4096,
 * det_cols < 5, a NaN or negative nms_thresh. */
int64_t dbx_nms_large_scratch_bytes(int32_t n);
int dbx_nms_large(const double* dets, int32_t n, int32_t det_cols, double nms_thresh, int32_t* keep, void* scratch, void* stream);

/* ---- pyramid merge: the rows of `levels` runs of dbx_detect_batch over the same `batch` frames (each run on the frames resized to
 * another size) mapped back to source-frame coordinates, and ONE greedy NMS per frame over their union -- one launch, one workgroup
 * per frame.
 * level_dets[l]: device rows [batch][K][det_cols] as dbx_detect_batch writes them.  xform[l * batch + b] maps level l's resized-frame
 * coordinates of frame b back to its source frame: x_src = x * scale - off_x, y_src = y * scale - off_y in float64, the product
 * rounded before the subtraction (no fused multiply-add): bit for bit NumPy's `d * scale - off`.
 * out_dets [batch][levels * K][det_cols]: row l * K + r of frame b is row r of level l with the x columns (0, 2, and 5, 7, 9, 11 when
 * det_cols == 13) and the y columns (1, 3, and 6, 8, 10, 12) mapped; column 4, the score, is copied; NaN rows pass through.
 * out_keep [batch][levels * K + 1]: per frame what dbx_nms returns on out_dets[b] (keep[0] = count; kept row numbers of out_dets[b] in
 * the reference's order; the level of a kept row is index / K) -- the same device code.
 * level_dets and xform are HOST arrays: the library copies its device records into `workspace` (device,
 * dbx_merge_nms_batch_workspace_bytes(levels, batch, K) bytes, which also holds every frame's NMS scratch) on `stream`, so the caller
 * may reuse them when the call returns and must keep `workspace` until the launch has run.  Refused with DBX_ERR_ARG before anything
 * is queued: levels, batch or K below 1, det_cols other than 5 or 13, a null pointer (any level pointer included), a scale that is not
 * finite and positive, a non-finite offset, levels * K above 4096 rows per frame (the rank pass of the NMS is quadratic in the row
 * count).  The workspace size is -1 for such counts. */
typedef struct dbx_merge_xform { double scale, off_x, off_y; } dbx_merge_xform;
int64_t dbx_merge_nms_batch_workspace_bytes(int32_t levels, int32_t batch, int32_t K);
int dbx_merge_nms_batch(const double* const* level_dets, const dbx_merge_xform* xform, int32_t levels, int32_t batch, int32_t K,
                        int32_t det_cols, double nms_thresh, double* out_dets, int32_t* out_keep, void* workspace, void* stream);

/* dbx_merge_nms_batch over VARIABLE row counts that never leave the device: level_dets[l] / level_counts[l] are what
 * dbx_thresh_rows_batch(max_dets) wrote for level l of the same `batch` frames (HOST arrays of device pointers, copied into `workspace`
 * like xform).  With n_(l,b) the count of level l, frame b -- read on the device, clamped to 0..max_dets, never trusted as a loop
 * bound -- frame b's union has m_b = sum over l of n_(l,b) rows.  Three launches on `stream` whose grids depend on (levels, batch,
 * max_dets) only; no host round trip, nothing polls.  Outputs (device), packed in dbx_detect_thresh_batch's style:
 *   out_counts  int32 [batch][levels][2]: the level pairs of every frame (the clamped n, the pixels above the threshold), then
 *               int32 [batch + 1]: P[b] = m_0 + ... + m_(b-1), P[batch] = the rows of the call.  2 * batch * levels + batch + 1 words.
 *   out_dets    frame b's m_b rows start at row P[b], level by level in the order of the levels, mapped as dbx_merge_nms_batch maps
 *               them (xform[l * batch + b]; column 4 copied; NaN passes through).  Capacity batch * levels * max_dets rows.
 *   out_keep    frame b's list is m_b + 1 words at word P[b] + b: the count, then the kept row numbers within the frame's union in
 *               the reference's order -- what dbx_nms_large returns on those m_b rows (score descending, the HIGHER union row first
 *               among equal scores, !(ovr <= thresh) suppresses).  out_keep == (int32_t*)out_dets asks for the lists right BEHIND
 *               the packed rows, at byte P[batch] * det_cols * 8 of out_dets: rows and lists are then
 *               P[batch] * (det_cols * 8 + 4) + batch * 4 contiguous bytes.
 * A frame with m_b == 0 writes its pairs, its prefix word and a zero list count, and nothing else.
 * workspace: dbx_merge_nms_thresh_batch_workspace_bytes(levels, batch, max_dets) bytes (device records, and per frame the NMS order
 * and the suppression matrix; -1 for counts out of range); it may be reused by the next call on the same stream.  Refused with
 * DBX_ERR_ARG before anything is queued: a null pointer (any level pointer included), levels or batch below 1, max_dets outside
 * 1..4096, levels * max_dets above 4096, det_cols other than 5 or 13, a scale that is not finite and positive, a non-finite offset,
 * a NaN or negative nms_thresh. */
int64_t dbx_merge_nms_thresh_batch_workspace_bytes(int32_t levels, int32_t batch, int32_t max_dets);
int dbx_merge_nms_thresh_batch(const double* const* level_dets, const int32_t* const* level_counts, const dbx_merge_xform* xform,
                               int32_t levels, int32_t batch, int32_t max_dets, int32_t det_cols, double nms_thresh,
                               double* out_dets, int32_t* out_keep, int32_t* out_counts, void* workspace, void* stream);

/* ---- tiled detection: a large frame cut into overlapping fixed-size windows ("tiles", optionally magnified), all tiles of all frames
 * run through one fixed-shape batched forward, and the rows stitched back per frame on the device.
 *
 * dbx_tile is one tile of a call's plan (64 bytes; offsets in brackets):
 *   frame [0]             index of the frame the tile was cut from; the tiles of frame b are a contiguous range of the table
 *   x0, y0 [4, 8]         window origin in the frame (>= 0): tile coordinate (x, y) is frame coordinate (x * scale + x0, y * scale + y0)
 *   side [12]             window side in source pixels (`src`)
 *   cw, ch [16, 20]       the part of the window inside the frame (min(side, W - x0), min(side, H - y0)); the rest of the window, on
 *                         the right / bottom only, is constant padding of 128
 *   scale [24]            src / tile as a double (tile: the network input side the window is resized to); < 1 magnifies
 *   lo2x, hi2x, lo2y, hi2y [32, 40, 48, 56]   the tile's CORE, the part of the plane it owns, as DOUBLED coordinates so that the
 *                         midpoint of an overlap is an integer: a box is owned iff lo2x <= x1 + x2 < hi2x and lo2y <= y1 + y2 < hi2y.
 *                         The first core of an axis starts at -inf, the last ends at +inf; cores are half-open and partition the plane.
 *
 * dbx_tile_grid (HOST function, no GPU): the plan of ONE h x w frame for window side `src` and `overlap` (source pixels), row-major
 * (y outer, x inner).  Along an axis of length L with stride D = src - overlap: L <= src gives one window at 0 (padded); otherwise
 * n = ceil((L - src) / D) + 1 windows start at s_i = min(i * D, L - src) (the last one shifted inward, nothing padded).  The core
 * boundary between windows i and i + 1 is m2_i = s_i + src + s_(i+1), the doubled midpoint of their overlap.  Writes frame = 0 and
 * scale = 1 (the caller sets both) and returns the tile count; out == NULL returns the count alone.  Refused with DBX_ERR_ARG:
 * src < 1, overlap < 0, 2 * overlap > src, h or w below 1, a non-null out with cap below the count, a plan of more than 2^20 tiles. */
#define DBX_TILE_RULE_NONE 0
#define DBX_TILE_RULE_CORE 1
typedef struct dbx_tile {
    int32_t frame, x0, y0, side, cw, ch;
    double  scale, lo2x, hi2x, lo2y, hi2y;
} dbx_tile;
int dbx_tile_grid(int32_t h, int32_t w, int32_t src, int32_t overlap, dbx_tile* out, int32_t cap);

/* The stitch.  `tiles` is the HOST table of the call's n_tiles tiles (checked before anything is queued), `tiles_dev` the caller's
 * DEVICE copy of the same bytes, which the kernels read (as data: nothing in it is trusted as a bound).  `stage` is the call's staging
 * area on the device, dbx_tile_stage_bytes(n_tiles, rows_per_tile, det_cols) bytes (-1 for counts out of range), in SLOT layout:
 *   int32  [n_tiles][2]                          per tile (rows delivered, rows owned)            (rounded up to 256 bytes)
 *   int32  [n_tiles][rows_per_tile]              the mark of every row: 1 owned, 0 not            (rounded up to 256 bytes)
 *   double [n_tiles][rows_per_tile][det_cols]    the rows in source-frame coordinates
 * Slots past a tile's delivered count are not written.
 *
 * dbx_tile_rows_batch, ONE launch per forward chunk: `rows` / `counts` are what dbx_detect_batch(K = rows_per_tile) -- rows
 * [n][rows_per_tile][det_cols], counts NULL: every tile delivers rows_per_tile rows -- or dbx_thresh_rows_batch(max_dets =
 * rows_per_tile) -- the same slot layout plus int32 counts [n][2], read on the device, clamped to 0..rows_per_tile and never trusted as
 * a loop bound -- wrote for tiles t0 .. t0 + n - 1 of the table.  Every delivered row goes to its slot of `stage` with the x columns
 * (0, 2, and 5, 7, 9, 11 when det_cols == 13) as x * scale - off_x, off_x = -x0, and the y columns alike, in float64 with the product
 * rounded before the subtraction (NumPy's `d * scale - off` bit for bit); column 4, the score, is copied; NaN passes through.  The
 * mark: under DBX_TILE_RULE_CORE the core test above on the MAPPED box in float64 (a NaN box is not owned); under DBX_TILE_RULE_NONE
 * every row is owned.  `rows` may be overwritten as soon as the launch has run: stream order is the only synchronisation.
 *
 * dbx_tile_nms_batch, once per call behind the last chunk: frame b's tiles are the range [first_b, first_(b+1)) of the table (T_b may
 * differ per frame); its owned rows are packed in tile order, then row order within the tile, and the reference's greedy NMS runs
 * over them with dbx_nms_large's semantics and device code (score descending, the HIGHER packed row first among equal scores,
 * !(ovr <= thresh) suppresses).  Three launches whose grids depend on (frames, n_tiles, rows_per_tile, the largest T_b) only: no host
 * round trip, nothing polls, and the call may be captured.  Outputs (device), packed as dbx_merge_nms_thresh_batch packs:
 *   out_counts  int32 [n_tiles][2]: the pairs of the staging area, then int32 [frames + 1]: P[b] = the owned rows of the frames before
 *               b, P[frames] = the rows of the call.  2 * n_tiles + frames + 1 words.
 *   out_dets    frame b's m_b owned rows start at row P[b].  Capacity n_tiles * rows_per_tile rows.
 *   out_keep    frame b's list is m_b + 1 words at word P[b] + b: the count, then the kept row numbers within the frame's packed rows.
 *               out_keep == (int32_t*)out_dets asks for the lists right BEHIND the packed rows, at byte P[frames] * det_cols * 8.
 *   out_tile    int32, packed like the rows: the index in the table of the tile each row came from.
 * A frame with no owned rows writes its pairs, its prefix word and a zero list count, and nothing else.
 * workspace: dbx_tile_nms_batch_workspace_bytes(frames, max_tiles, rows_per_tile) bytes with max_tiles the largest T_b (-1 when
 * max_tiles * rows_per_tile exceeds 4096 or a count is out of range).
 * Refused with DBX_ERR_ARG before anything is queued: null pointers (counts excepted), n_tiles, n or frames below 1, t0 < 0 or
 * t0 + n > n_tiles, det_cols other than 5 or 13, rows_per_tile outside 1..4096, a rule other than the two, any frame with
 * T_b * rows_per_tile > 4096 (the NMS's bound), a tile with a scale that is not finite and positive, a negative origin or a NaN core
 * bound, a table whose frame indices are not non-decreasing within 0..frames-1, a NaN or negative nms_thresh.
 *
 * dbx_tile_host runs the kernels' own mapping and ownership code on the CPU (no GPU needed): row i of rows [n][det_cols] is mapped by
 * tiles[tile_of[i]] into out_rows [n][det_cols]; op 1 also writes its mark under `rule` to out_marks [n] (op 0: the map alone). */
int64_t dbx_tile_stage_bytes(int32_t n_tiles, int32_t rows_per_tile, int32_t det_cols);
int dbx_tile_rows_batch(const double* rows, const int32_t* counts, const dbx_tile* tiles, const dbx_tile* tiles_dev, int32_t n_tiles,
                        int32_t t0, int32_t n, int32_t rows_per_tile, int32_t det_cols, int32_t rule, void* stage, void* stream);
int64_t dbx_tile_nms_batch_workspace_bytes(int32_t frames, int32_t max_tiles, int32_t rows_per_tile);
int dbx_tile_nms_batch(const dbx_tile* tiles, const dbx_tile* tiles_dev, int32_t n_tiles, int32_t frames, int32_t rows_per_tile,
                       int32_t det_cols, double nms_thresh, const void* stage, double* out_dets, int32_t* out_keep, int32_t* out_tile,
                       int32_t* out_counts, void* workspace, void* stream);
int dbx_tile_host(int32_t op, int64_t n, const dbx_tile* tiles, int32_t n_tiles, const int32_t* tile_of, const double* rows,
                  int32_t det_cols, int32_t rule, double* out_rows, int32_t* out_marks);

/* ---- plate rectification after decode (perspective_transform, DenseBox.py:3446-3481; OpenCV's published algorithm) ----
 * dbx_perspective_matrix: host function, cv2.getPerspectiveTransform: 3x3 row-major double map src -> dst of four (x, y)
 *   float pairs.  dbx_warp_perspective_u8: cv2.warpPerspective(img, M, (dw, dh)) with INTER_LINEAR and a zero border on an
 *   interleaved uint8 image [h][w][c] (device pointers). */
int dbx_perspective_matrix(const float* src_xy, const float* dst_xy, double* m9);
int dbx_warp_perspective_u8(const uint8_t* src, int32_t sh, int32_t sw, int32_t c, const double* m9, uint8_t* dst,
                            int32_t dh, int32_t dw, void* stream);
/* Batched warp: one launch over njobs jobs.  A job is one (source image, map, output window): it writes canvas rows y0..y0+oh-1,
 * columns x0..x0+ow-1 of what dbx_warp_perspective_u8(src, sh, sw, c, m9, ., dh, dw) would write -- the same bits -- as a
 * contiguous [oh][ow][c] block at byte offset dst_off of `dst` (64-bit offsets: arenas above 2 GiB are fine; any dst_off works, and
 * a 16-byte aligned dst + dst_off is stored in 16-byte words for every c, a 4-byte aligned one in dwords, others byte by byte).  Jobs may read different images of different sizes; all share the channel count c (1..4).
 * `jobs` is a HOST array: the library inverts every m9 and copies the device records into `workspace` (device,
 * dbx_warp_batch_workspace_bytes(njobs) bytes) on `stream`, so the caller may reuse `jobs` when the call returns and must keep
 * `workspace` until the launch has run.  Refused with DBX_ERR_ARG before anything is queued: njobs < 0, c outside 1..4, a null
 * pointer, a non-positive size, a window outside its canvas, a negative dst_off, a non-finite or singular m9, more pixels than one
 * grid holds (2^24 - 1 workgroups of 2048 pixels).  njobs == 0: no-op. */
typedef struct dbx_warp_job {
    const uint8_t* src;      /* device image [sh][sw][c] */
    int32_t sh, sw;
    double m9[9];            /* forward map src -> canvas, as for dbx_warp_perspective_u8 */
    int32_t dh, dw;          /* canvas size (cv2 dsize) */
    int32_t x0, y0, oh, ow;  /* window written: canvas rows y0..y0+oh-1, cols x0..x0+ow-1 */
    int64_t dst_off;         /* byte offset of this job's [oh][ow][c] output in dst */
} dbx_warp_job;
int64_t dbx_warp_batch_workspace_bytes(int32_t njobs);
int dbx_warp_perspective_batch_u8(const dbx_warp_job* jobs, int32_t njobs, int32_t c, uint8_t* dst, void* workspace, void* stream);

/* Fixed-size plate crops, rectified on the device: one launch over nframes x slots crops of oh x ow pixels, with no host work between
 * the decode and the warp.  Everything the launch reads is on the DEVICE or passed by value; the call copies nothing from the host and
 * never synchronises, so it can be captured into a hipGraph behind dbx_detect_batch.
 *   frames      device table of nframes records {src, sh, sw}: interleaved uint8 images [sh][sw][c] of any sizes (the caller uploads it)
 *   quads       device float64; the 8 values (x_lu, y_lu, x_ru, y_ru, x_rd, y_rd, x_ld, y_ld) of row r of frame b are at
 *               quads + b * frame_stride + r * row_stride (strides in doubles).  Detection rows: dets + 5, row_stride 13,
 *               frame_stride K * 13
 *   sel         device int32 [nframes][slots + 1] in dbx_detect_batch's `keep` layout: the count, then the row indices in that order
 *               (slot j is row sel[b][1 + j]); NULL: rows 0..slots-1.  A count is clamped to 0..slots; a row index that is negative or
 *               whose quad does not end inside the frame's stride (r * row_stride + 8 > frame_stride) makes the slot not ok
 *   dst         device uint8 [nframes][slots][oh][ow][c]; ok: device int32 [nframes][slots]
 *   m9_out      optional device float64 [nframes][slots][9] (may be NULL): the forward matrix of every slot that is ok; entries of
 *               other slots are not written
 * Slot (b, j) with j below the count: every coordinate is rounded to float32 and widened again; the map is dbx_perspective_matrix's
 * solve (the same function, compiled for the device) from the quad to the rectangle (0,0), (ow-1,0), (ow-1,oh-1), (0,oh-1) as float32
 * values (corners on the centres of the first and last pixel); its inverse and every pixel are dbx_warp_perspective_u8's, so a crop is
 * bit for bit dbx_warp_perspective_u8(src, sh, sw, c, m9, ., oh, ow) with the host's m9.  A slot is NOT ok (ok = 0, crop all zeros)
 * when a float32 coordinate is not finite, a pivot fails dbx_perspective_matrix's test, an entry of the matrix is not finite, the
 * cofactor determinant is 0.0, or its frame record has a null src or a non-positive size; so are the slots past the count.  The call
 * writes every byte of dst and every word of ok (16-byte words where a slot's address allows, dwords or bytes otherwise) and nothing
 * outside them.  It needs no workspace.
 * Refused with DBX_ERR_ARG before anything is queued: nframes < 0, c outside 1..4, slots < 1, ow or oh < 1, row_stride < 8,
 * frame_stride < slots * row_stride when sel is NULL, a null frames / quads / dst / ok, more tiles than one grid holds (2^24 - 1
 * workgroups of 2048 pixels, ceil(oh * ow / 2048) per slot).  nframes == 0: no-op. */
typedef struct dbx_crop_frame {
    const uint8_t* src;      /* device image [sh][sw][c] */
    int32_t sh, sw;
} dbx_crop_frame;
int dbx_plate_crops_batch(const dbx_crop_frame* frames, int32_t nframes, int32_t c, const double* quads, int64_t row_stride,
                          int64_t frame_stride, const int32_t* sel, int32_t slots, int32_t ow, int32_t oh, uint8_t* dst, int32_t* ok,
                          double* m9_out, void* stream);

/* ---- evaluation behind decode + NMS (no reference counterpart: its test* drivers only draw; the matching is the PASCAL VOC devkit's
 * with the +1-pixel IoU of the reference's NMS, DenseBox.py:3398-3443) ----
 * dbx_match_gt_batch: one launch, a workgroup per frame; it copies nothing from the host and never synchronises, so it can be captured
 * into a hipGraph behind the decode.  Rows and lists are read where the decode left them:
 *   prefix == NULL  dbx_detect_batch's slot layout: frame b's rows start at row b * slots of dets, its keep list is the slots + 1 words
 *                   at keep + b * (slots + 1); det_rows >= batch * slots.
 *   prefix != NULL  dbx_detect_thresh_batch's packed layout with slots = its max_dets: prefix is the device int32 [batch + 1] that call
 *                   leaves at counts + 2 * batch; frame b's n_b = P[b + 1] - P[b] rows start at row P[b], its list is at word P[b] + b of
 *                   keep (the address the decode wrote its lists to; det_rows + batch words).
 *   det_rows        the capacity of dets in rows of det_cols (5 or 13) float64.
 * The detections of a frame are its kept rows in list order, numbered i = 0..k-1 by position.  gt: float64 [batch][max_gt][gt_cols],
 * a box (x1, y1, x2, y2) in the rows' coordinates and, with gt_cols == 12, a quad of 8 values in the order of row columns 5..12;
 * gt_counts int32 [batch], clamped to 0..max_gt; gt_ignore uint8 [batch][max_gt] or NULL (no box is ignored).
 * IoU in float64, the NMS's formula: areas (x2 - x1 + 1) * (y2 - y1 + 1), intersection sides max(0, min(x2) - max(x1) + 1), ovr = inter /
 * (area_d + area_g - inter), the product rounded before the subtraction.  For detection i: jmax = the GT of the largest ovr (the lowest
 * index on ties; a NaN ovr never wins), ovmax = that ovr (-inf without one); matched when ovmax > iou_thresh, strictly.  status 0 (FP) and
 * gt_index -1 when not matched; status -1 (ignored) and gt_index jmax when jmax carries the ignore flag; status 1 (TP) when i is the
 * first detection in list order matched to jmax, else status 0 (duplicate FP), both with gt_index jmax.  Outputs (device), in slot
 * layout by list position:
 *   status, gt_index  int32 [batch][slots]: EVERY word is written; positions past the list count get status -2 and gt_index -1.
 *   iou               float64 [batch][slots]: ovmax, positions below the count only.
 *   lm_err            float64 [batch][slots] or NULL; a pointer needs det_cols == 13 && gt_cols == 12.  For a TP the mean over the four
 *                     corners of the distance between the row's landmark and the GT's, over sqrt of the GT box's area; NaN otherwise;
 *                     positions below the count only.
 *   tally             int32 [batch][5]: (counted positions, TP, FP, ignored, GT boxes without the ignore flag), every word written.
 * Whatever the device data says, nothing outside the buffers is read: a keep count is clamped to 0..min(slots, n_b); a frame whose
 * prefix pair is negative, decreasing or ends beyond det_rows is empty; a keep entry outside 0..n_b-1 gives its position status -2
 * (iou and lm_err NaN) and the position is not counted.  GT boxes and the per-GT claim words live in LDS (45 bytes per GT); there is no
 * scratch buffer.  Refused with DBX_ERR_ARG before anything is queued: batch < 0, det_cols other than 5 or 13, gt_cols other than 4 or
 * 12, slots outside 1..4096, max_gt outside 1..1024, det_rows < 0 or (slot layout) below batch * slots, a NaN iou_thresh, lm_err with
 * other columns than 13 / 12, a null pointer (prefix, gt_ignore and lm_err excepted).  batch == 0: no-op.
 *
 * dbx_eval_append: one small launch behind the match, capturable likewise.  Every counted position of the call becomes a record, in
 * frame order, then list order, at records[cursor...]; the running totals are updated; the result does not depend on scheduling.
 * The dets / keep / prefix / slots description is the match's; status, lm_err (may be NULL: the records hold NaN) and tally are what the
 * match wrote.  state: device int64 [8] = {cursor, dropped, frames, n_gt, tp, fp, ignored, reserved}, zero before the first call.
 * record.frame = the running frame number, state.frames + b.  Records past `capacity` are not written and are counted in dropped; the
 * totals take the whole tallies.  Refused: the match's refusals of the shared arguments, capacity < 0, a null pointer (prefix and lm_err
 * excepted; records only when capacity is 0).  batch == 0: no-op.
 * The record is 24 bytes: score at 0, lm_err at 8, status at 16, frame at 20. */
typedef struct dbx_eval_record {
    double  score;     /* column 4 of the row */
    double  lm_err;    /* NaN unless a TP matched with landmarks */
    int32_t status;    /* 1 TP, 0 FP, -1 ignored */
    int32_t frame;     /* running frame number of the evaluation pass */
} dbx_eval_record;
int dbx_match_gt_batch(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                       int32_t batch, int32_t slots, const double* gt, int32_t gt_cols, const int32_t* gt_counts,
                       const uint8_t* gt_ignore, int32_t max_gt, double iou_thresh, int32_t* status, int32_t* gt_index,
                       double* iou, double* lm_err, int32_t* tally, void* stream);
int dbx_eval_append(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                    int32_t batch, int32_t slots, const int32_t* status, const double* lm_err, const int32_t* tally,
                    dbx_eval_record* records, int64_t capacity, int64_t* state, void* stream);

/* ---- multi-stream tracking behind decode + NMS (no reference counterpart: tracking by detection with an alpha-beta filter per box
 * coordinate and greedy IoU association, the +1-pixel IoU of the reference's NMS, DenseBox.py:3398-3443) ----
 * dbx_track_update_batch: one launch, a workgroup per frame; it copies nothing from the host and never synchronises, so it can be captured
 * into a hipGraph behind the decode.  Frame b of the launch belongs to stream stream0 + b, so a launch never holds two frames of one
 * stream.  dets / det_cols / det_rows / keep / prefix / batch / slots describe the rows and keep lists exactly as for dbx_match_gt_batch
 * (slot layout when prefix == NULL, dbx_detect_thresh_batch's packed layout otherwise), with slots in 1..1024.
 * State (device): headers int32 [streams][4] = {frame, next_id, unborn, reserved} and tracks dbx_track [streams][max_tracks]; id < 0
 * marks a free slot, whatever else it holds; all-zero headers with all ids -1 are the initial state.
 * Stream s at its frame number f = header.frame; the detections are the kept rows in list order, i = 0..k-1:
 *   A  predict   every live slot t: p_t = box_t + vel_t (four additions).
 *   B  associate for i ascending, over the live slots not yet claimed in this frame: ovr(p_t, row_i) by the NMS's formula as
 *                dbx_match_gt_batch states it (+1 sides, the product rounded before the subtraction); the winner is the slot of the
 *                largest ovr, the lowest slot index on ties, a NaN ovr never wins; the slot is claimed by i when that ovr > iou_thresh,
 *                strictly.  Slots born in D are never candidates in the same frame.
 *   C  update    every live slot in ascending slot order.  Claimed by i: r = row_i.box - p; box = p + alpha * r; vel = vel + beta * r;
 *                score = row_i[4]; if score > best_score (strictly): best_score = score, best_frame = f; hits += 1, age = 0,
 *                last_frame = f.  Unclaimed: box = p, age += 1, and when age > max_age the slot is retired: its record is copied to
 *                retired[b][n++] (ascending slot order) and its id in the table set to -1 (the rest of the slot keeps the record).
 *   D  births    unmatched detections in list order.  Born when all four coordinates are finite, row[4] >= birth_score (a NaN score
 *                fails) and a free slot exists; it takes the lowest free index, slots freed in C included; id = next_id++, box =
 *                row.box, vel = 0, score = best_score = row[4], hits = 1, age = 0, first_frame = last_frame = best_frame = f.
 *                Otherwise the detection gets no track and header.unborn += 1.
 *   E            header.frame = f + 1.
 * Outputs (device), slot layout by list position:
 *   track_id    int32 [batch][slots]: EVERY word is written; the track's id, -1 for a counted position without a track, -2 for positions
 *               past the count and for a keep entry outside 0..n_b-1, which is not counted.
 *   track_slot  int32 [batch][slots]: EVERY word is written; the slot index, -1 wherever track_id < 0.
 *   track_hits  int32 [batch][slots]: the track's hits after the update (0 wherever track_id < 0); positions below the count only.
 *   retired     dbx_track [batch][max_tracks]: the first tally[b][4] records of each frame.
 *   tally       int32 [batch][6]: (counted positions, matched, born, unborn, retired, live after), every word written.
 * Whatever the device data says, nothing outside the buffers is read or written: a keep count is clamped to 0..min(slots, n_b); a frame
 * whose prefix pair is negative, decreasing or ends beyond det_rows has no detections and its tracks coast.  One thread per track slot
 * keeps the slot's record in registers; LDS holds 44 bytes per list position (box, score, the slot it ended up with) and 16 bytes per
 * track slot (free-list entry, birth, id and hits for the outputs): 48 KB at the limits; there is no scratch buffer.
 * Refused with DBX_ERR_ARG before anything is queued: batch < 0, stream0 < 0, stream0 + batch > streams, det_cols other than 5 or 13,
 * slots outside 1..1024, max_tracks outside 1..256, max_age < 0, a NaN iou_thresh, alpha, beta or birth_score, det_rows < 0 or (slot
 * layout) below batch * slots, a null pointer (prefix excepted).  batch == 0: no-op.
 *
 * dbx_track_append: one small launch behind the update, capturable likewise.  The retired records of the call go to records[cursor...]
 * in frame order, then `retired` order, with stream = stream0 + b; the result does not depend on scheduling.  retired and tally are what
 * the update wrote (tally[b][4] is clamped to 0..max_tracks).  state: device int64 [4] = {cursor, dropped, retired_total, reserved},
 * zero before the first call.  Records past `capacity` are not written and are counted in dropped; retired_total counts them all.
 * Refused: batch < 0, stream0 < 0, max_tracks outside 1..256, capacity < 0, a null pointer (records only when capacity is 0).
 * batch == 0: no-op.
 * dbx_track is 104 bytes (box at 0, vel at 32, score at 64, best_score at 72, the six int32 from 80); dbx_track_record is 112 bytes
 * (stream at 0, reserved at 4, the track at 8). */
typedef struct dbx_track {
    double  box[4];        /* x1, y1, x2, y2 after the last update (the prediction while coasting) */
    double  vel[4];        /* per-coordinate velocity, pixels per frame */
    double  score;         /* column 4 of the last matched row */
    double  best_score;    /* the largest score seen, and the frame it was seen in (best_frame) */
    int32_t id;            /* >= 0 live, < 0 free */
    int32_t hits;          /* detections matched to the track, its birth included */
    int32_t age;           /* frames since the last match */
    int32_t first_frame;
    int32_t last_frame;    /* the frame of the last match */
    int32_t best_frame;
} dbx_track;
typedef struct dbx_track_record {
    int32_t   stream;
    int32_t   reserved;
    dbx_track t;
} dbx_track_record;
int dbx_track_update_batch(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                           int32_t batch, int32_t slots, int32_t* headers, dbx_track* tracks, int32_t streams, int32_t stream0,
                           int32_t max_tracks, double iou_thresh, int32_t max_age, double alpha, double beta, double birth_score,
                           int32_t* track_id, int32_t* track_slot, int32_t* track_hits, dbx_track* retired, int32_t* tally, void* stream);
int dbx_track_append(const dbx_track* retired, const int32_t* tally, int32_t batch, int32_t max_tracks, int32_t stream0,
                     dbx_track_record* records, int64_t capacity, int64_t* state, void* stream);

/* ---- best-shot gallery behind the crops and the tracking update (no reference counterpart): per track the best plate crop the camera
 * ever saw of it, kept on the device until the track ends ----
 * dbx_crop_sharpness: out[i] = the focus measure of crop i of crops uint8 [n][oh][ow][c], one workgroup per crop.  c is 1 or 3; the
 * luma is Y = 4 * v (c == 1) or Y = c0 + 2 * c1 + c2 (c == 3), the same for RGB and BGR, at most 1020; for every interior pixel
 * L = 4 * Y(y, x) - Y(y-1, x) - Y(y+1, x) - Y(y, x-1) - Y(y, x+1), and out[i] is the sum of L * L over the interior in 64-bit integer
 * arithmetic (0 when oh < 3 or ow < 3): exact, whatever the order of the reduction.  The luma plane is staged in LDS as 16-bit values,
 * hence oh * ow <= 16384; the sum goes per thread, then by wave shuffle, then across the waves through LDS; there are no atomics.
 * Refused with DBX_ERR_ARG before anything is queued: n < 0, c other than 1 or 3, oh or ow < 1, oh * ow > 16384, a null pointer.
 * n == 0: no-op.
 *
 * dbx_track_gallery_update: one launch, a workgroup of 256 threads per (track slot t, frame b) on a grid of (max_tracks, batch); it
 * copies nothing from the host and never synchronises, so it can be captured into a hipGraph.  It runs BEHIND dbx_track_update_batch and
 * dbx_plate_crops_batch of the same frames and BEFORE dbx_track_append of the same call, so that it reads the append cursor as it stood
 * before the call.  Inputs (device): tracks and headers as the update left them; track_slot int32 [batch][slots]; crops uint8
 * [batch][slots][oh][ow][c] and ok int32 [batch][slots], both by list position, as dbx_plate_crops_batch writes them with sel = keep;
 * retired dbx_track [batch][max_tracks] and tally int32 [batch][6] as the update wrote them; append_state, dbx_track_append's int64 [4],
 * of which only word 0, the cursor, is read.  Gallery state (device): shots dbx_shot [streams][max_tracks]; shot_crops uint8
 * [streams][max_tracks][oh][ow][c]; arena dbx_shot_record [capacity], every shot.id -1 initially; arena_crops uint8
 * [capacity][oh][ow][c]; gstate int64 [4] = {ended, stored, lost, dropped}.  A free entry of shots has id = -1; a fresh entry for track
 * id i has key = -inf, score = NaN, sharpness = 0, id = i, frame = -1, shots = 0, reserved = 0.
 * For stream s = stream0 + b and slot t, with G = shots[s][t], K = tracks[s][t], f = headers[s].frame - 1 and R_b = tally[b][4] clamped
 * to 0..max_tracks:
 *   1  ended      G.id >= 0 and K.id != G.id: ended += 1.  n = the lowest index below R_b with retired[b][n].id == G.id.  Found: i =
 *                 cursor + sum of R_b' over b' < b + n, the index dbx_track_append is about to give that record; when the cursor is
 *                 not negative and i < capacity, arena[i] = {s, t, G}, arena_crops[i] = shot_crops[s][t] and stored += 1, otherwise
 *                 dropped += 1.  Not found (the tracker was advanced without the gallery in between): lost += 1.  In every case
 *                 G.id = -1.
 *   2  adoption   K.id >= 0 and G.id != K.id: G becomes the fresh entry for K.id and shot_crops[s][t] is zeroed.  A slot retired and
 *                 reborn in one frame passes through 1 and 2 in that order.
 *   3  candidate  K.id >= 0 and a list position j has track_slot[b][j] == t (the lowest such j below slots).  The crop is a candidate
 *                 when ok[b][j] != 0 and K.score >= min_score (a NaN score fails; K.score is the row's score, which the update stored
 *                 for every track matched or born in this frame).  Then S = the sharpness of crops[b][j], key = (double)S under policy
 *                 0 or K.score under policy 1, G.shots += 1, and when this is the first candidate (shots was 0) or key > G.key,
 *                 strictly: G.key = key, G.score = K.score, G.sharpness = S, G.frame = f and shot_crops[s][t] = the crop (16-byte
 *                 words where the addresses allow).  A live track without a list position coasts and is left alone.
 * The counters are integer adds, one per counter and workgroup at most; nothing else depends on scheduling.  commit == 0: the launch
 * does all its reads and the reduction and writes nothing (the warm-up runs of a graph capture).  Whatever the device data says,
 * nothing outside the buffers is read or written: R_b is clamped, a track_slot entry outside 0..max_tracks-1 names no slot, a negative
 * cursor is a drop.  LDS: the luma plane and 64 bytes; there is no scratch buffer.
 * Refused with DBX_ERR_ARG before anything is queued: batch < 0, stream0 < 0, stream0 + batch > streams, slots outside 1..1024,
 * max_tracks outside 1..256, c other than 1 or 3, oh or ow < 1, oh * ow > 16384, capacity < 0, policy other than 0 or 1, a NaN
 * min_score, a null pointer (arena and arena_crops only when capacity is 0), batch above 65535 (one grid).  batch == 0: no-op.
 * dbx_shot is 40 bytes (key at 0, score at 8, sharpness at 16, the four int32 from 24); dbx_shot_record is 48 bytes (stream at 0, slot
 * at 4, the shot at 8). */
typedef struct dbx_shot {
    double  key;           /* what the shots are ranked by: (double)sharpness under policy 0, score under policy 1; -inf without a shot */
    double  score;         /* the track's score in the frame of the shot; NaN without a shot */
    int64_t sharpness;     /* dbx_crop_sharpness of the shot */
    int32_t id;            /* the track's id; < 0 free */
    int32_t frame;         /* the stream's frame number of the shot; -1 without a shot */
    int32_t shots;         /* candidates seen */
    int32_t reserved;
} dbx_shot;
typedef struct dbx_shot_record {
    int32_t  stream;
    int32_t  slot;
    dbx_shot shot;
} dbx_shot_record;
int dbx_crop_sharpness(const uint8_t* crops, int64_t n, int32_t oh, int32_t ow, int32_t c, int64_t* out, void* stream);
int dbx_track_gallery_update(const dbx_track* tracks, const int32_t* headers, const int32_t* track_slot, const uint8_t* crops,
                             const int32_t* ok, const dbx_track* retired, const int32_t* tally, const int64_t* append_state,
                             dbx_shot* shots, uint8_t* shot_crops, dbx_shot_record* arena, uint8_t* arena_crops, int64_t* gstate,
                             int32_t batch, int32_t slots, int32_t streams, int32_t stream0, int32_t max_tracks, int32_t oh, int32_t ow,
                             int32_t c, int64_t capacity, int32_t policy, double min_score, int32_t commit, void* stream);

/* ---- annotated frames (viz_result, DenseBox.py:3484-3560: cv2.rectangle, the filled label + cv2.putText, cv2.circle per landmark, the
 * rectified plate shown next to the frame) painted on the device behind the decode, the plate crops and the tracking update ----
 * The layout, default colours, thickness, radius and anchor points follow viz_result; the pixel semantics below are this project's own,
 * restated in NumPy by tests/viz_ref.py.  OpenCV is not part of the reference tree: parity with cv2.rectangle / putText / circle is
 * unpinned.
 * dbx_draw_overlay_batch: ONE launch, a workgroup of 256 threads per 128 x 16 tile of a frame on a grid of (the tiles of a max_h x
 * max_w frame, batch); it copies nothing from the host and never synchronises, so it can be captured into a hipGraph behind the decode,
 * dbx_plate_crops_batch and dbx_track_update_batch.
 * frames: a DEVICE table of `batch` records; frame b is an interleaved uint8 [h][w][c] image of any size up to max_h x max_w, read at
 * src and written at dst.  dst == src draws in place; any other overlap is the caller's error.  dets / det_cols / det_rows / keep /
 * prefix / slots: the description dbx_match_gt_batch and dbx_track_update_batch take (prefix == NULL: slot layout; otherwise the packed
 * layout of dbx_detect_thresh_batch).  track_id: int32 [batch][slots] by list position, as dbx_track_update_batch writes it, or NULL.
 * crops uint8 [batch][slots][oh][ow][c] and ok int32 [batch][slots], by list position, as dbx_plate_crops_batch writes them with sel =
 * keep; both NULL: no inset.
 * Notation: I(v) = v + 0.5 in float64, truncated toward zero; T(v) = v truncated toward zero; a value is usable when it is finite and
 * |v| < 2^30.
 * Everything is clipped to the frame.  Within a frame the kept rows are painted in list order, later over earlier; within a row the
 * order is outline, label background, label text, discs 0..3, inset; a pixel nothing covers is src's.  So every dst pixel is a function
 * of the inputs alone, not of scheduling.  A row whose x1, y1, x2, y2 (columns 0..3) are not all usable paints nothing.  X1 = I(x1), Y1,
 * X2, Y2 likewise; L, R = min, max(X1, X2); Tp, Bt = min, max(Y1, Y2); t = thickness, a = t / 2 (integer), b = t - a.
 *   outline  (box colour) L-a <= x <= R+a, Tp-a <= y <= Bt+a, except the pixels with L+b <= x <= R-b and Tp+b <= y <= Bt-b.
 *   label    when font_scale = s > 0: the text has n characters of a 6 x 8 cell, tw = 6 s n, th = 8 s.  Background (box colour):
 *            X1 <= x <= X1+tw+3, Y1-th-5 <= y <= Y1 (viz_result's pt_1 .. pt_1 + (w + 3, -h - 5)).  Text (text colour): a set font
 *            pixel (i, j) of character m covers the s x s block at x = X1 + 2 + (6 m + i) s, y = Y1 - 2 - th + j s.
 *   discs    (mark colour) when det_cols == 13 and radius = r >= 0: for q = 0..3 the centre is (T(row[5+2q]), T(row[6+2q])), both
 *            usable, else that disc is skipped; it covers dx*dx + dy*dy <= r*r.
 *   inset    when crops is given and ok[b][j] != 0 (j the list position): with m = inset_scale, px = L-a and py = Bt+a+2, the pixel
 *            (x, y) in [px, px + ow m) x [py, py + oh m) takes crops[b][j][(y-py)/m][(x-px)/m].
 * Text: "#", the id in decimal and a space when track_id is given and track_id[b][j] >= 0; then the score v = row[4]: when v is finite
 * and |v| < 1000, exactly what C's "%.3f" prints (the exact binary value correctly rounded, ties to even, "-" whenever the sign bit is
 * set: "-0.000"), computed in integer arithmetic on the double's bits; otherwise "---".  The characters are "0123456789.-# ".
 * Channel ch of a painted pixel takes color[ch] of its colour.
 * Device data is never trusted as a bound: keep counts are clamped to min(rows of the frame, slots), a keep entry outside the frame's
 * rows paints nothing, a frame with a bad prefix pair has no rows and is copied undrawn; a frame record with a null src or dst, a
 * non-positive size, h > max_h or w > max_w is skipped and its dst not written.  For every other frame the call writes every byte of
 * dst (in place: every byte that changes) and nothing outside it.  A tile no row meets is moved with 16-byte accesses where src and dst
 * allow the same ones, bytes at the ragged ends.  LDS: 88 bytes per slot; there is no scratch buffer.
 * Refused with DBX_ERR_ARG before anything is queued: batch < 0, c outside 1..4, max_h or max_w < 1, det_cols not 5 or 13, slots
 * outside 1..1024, det_rows < 0 (or below batch * slots in slot layout), thickness outside 1..16, radius outside -1..32, font_scale
 * outside 0..8, inset_scale outside 1..8, exactly one of crops / ok null, crops with ow or oh < 1, a null frames / dets / keep / style,
 * more than 2^24 - 1 tiles or 65535 frames (one grid).  batch == 0: no-op.
 * dbx_overlay_frame is 24 bytes (src 0, dst 8, h 16, w 20); dbx_overlay_style is 28 bytes (the three colours at 0, 4, 8, then thickness,
 * radius, font_scale, inset_scale from 12).
 *
 * The same text and font code compiled for the host (no GPU needed):
 * dbx_overlay_font: out uint8 [14][8], row j of glyph g of "0123456789.-# " in out[g][j], bit i = column i (5 x 7 in the 6 x 8 cell).
 * dbx_overlay_label: the label of (score, track_id; a negative id: none) as a NUL-terminated string in out; returns its length (at
 * most 21), or DBX_ERR_ARG when out is null or out_len < 22. */
typedef struct dbx_overlay_frame {
    const uint8_t* src;    /* device image [h][w][c] */
    uint8_t* dst;          /* device image [h][w][c]; may equal src */
    int32_t h, w;
} dbx_overlay_frame;
typedef struct dbx_overlay_style {
    uint8_t box_color[4], text_color[4], mark_color[4];    /* channel ch of a pixel takes color[ch] */
    int32_t thickness;     /* 1..16 */
    int32_t radius;        /* -1 (no discs) .. 32 */
    int32_t font_scale;    /* 0 (no label) .. 8 */
    int32_t inset_scale;   /* 1..8 */
} dbx_overlay_style;
int dbx_draw_overlay_batch(const dbx_overlay_frame* frames, int32_t batch, int32_t c, int32_t max_h, int32_t max_w,
                           const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix,
                           int32_t slots, const int32_t* track_id, const uint8_t* crops, const int32_t* ok, int32_t ow, int32_t oh,
                           const dbx_overlay_style* style, void* stream);
int dbx_overlay_font(uint8_t* out);
int dbx_overlay_label(double score, int32_t track_id, char* out, int32_t out_len);

/* ---- plate redaction (no reference counterpart): the frame with every plate made unreadable, written on the device behind the decode
 * and the tracking update.  The semantics are this project's own, restated in NumPy by tests/redact_ref.py ----
 * dbx_redact_batch: ONE launch, a workgroup of 256 threads per 64 x 16 tile of a frame on a grid of (the tiles of a max_h x max_w frame,
 * batch); it copies nothing from the host and never synchronises, so it can be captured into a hipGraph behind the decode and
 * dbx_track_update_batch.
 * frames: a DEVICE table of `batch` dbx_overlay_frame records, as for dbx_draw_overlay_batch: frame b is an interleaved uint8 [h][w][c]
 * image, read at src and written at dst.  dets / det_cols / det_rows / keep / prefix / slots: the decoded-rows description every such
 * entry point takes (prefix == NULL: slot layout; otherwise dbx_detect_thresh_batch's packed layout), slots in 1..1024.  tracks:
 * const dbx_track [streams][max_tracks] as dbx_track_update_batch left it, or NULL (streams, stream0 and max_tracks are then not read);
 * frame b belongs to stream stream0 + b.
 * Notation: I(v), T(v) and "usable" as for dbx_draw_overlay_batch.  All arithmetic is integer.
 * Regions of frame b:
 *   1  every kept row (the keep count clamped, a keep entry outside the frame's rows ignored, as everywhere else).  A row is skipped only
 *      when row[4] < min_score, so a NaN score is redacted.  A row whose x1, y1, x2, y2 are not all usable has no region.
 *   2  when tracks is given and coast > 0: every slot of the stream with id >= 0, 1 <= age <= coast and a usable box -- the coasting
 *      tracks, whose box is the prediction for a frame in which the detector missed the plate.  Always a box region.
 * Box region: L, R, Tp, Bt as in the overlay; gx = grow + ((R - L + 1) * grow_pct) / 100 and gy likewise on Bt - Tp + 1, in int64; the
 * region is L-gx <= x <= R+gx, Tp-gy <= y <= Bt+gy, clipped to the frame.
 * Quad region (shape == 1 and det_cols == 13): P_q = (I(row[5+2q]), I(row[6+2q])), q = 0..3.  The row falls back to its box region
 * when a landmark is not finite or has |v| >= 2^20, or when the shoelace sum of P_0..P_3 (the sum over q of Px_q Py_q+1 - Px_q+1 Py_q,
 * indices mod 4) is 0.  Otherwise, in quarter pixels and per axis: S = P_0 + P_1 + P_2 + P_3, d = 4 P_q - S,
 * G_q = 4 P_q + (d * grow_pct) / 100 + 4 * grow * sgn(d) (C's division, truncating toward zero), and the region is
 * tri(G_0, G_1, G_2) u tri(G_0, G_2, G_3) clipped to the frame: the pixel (x, y) is inside a triangle when its three int64 edge
 * functions at (4x, 4y), (b - a) x (p - a) for the edges a->b = G_i->G_j, G_j->G_k, G_k->G_i, multiplied by the sign of the triangle's
 * doubled area, are all >= 0; a triangle of zero area covers nothing.
 * Value: a pixel no region covers keeps src.  A covered pixel's value depends on src alone, so neither list order nor scheduling matters:
 *   fill      (method 0) dst[ch] = color[ch].
 *   pixelate  (method 1) cells of s = cell pixels anchored to the frame's origin: the cell of (x, y) is [s*(x/s), min(s*(x/s)+s, w)) x
 *             [s*(y/s), min(s*(y/s)+s, h)), of n pixels; dst[ch] = (sum of src[ch] over the cell + n/2) / n.  Pixels of the cell
 *             outside every region count in the sum.
 *   blur      (method 2) r = radius, A = (2r+1)^2: dst[ch] = (sum over dy, dx in [-r, r] of src[clamp(y+dy, 0, h-1)][clamp(x+dx, 0,
 *             w-1)][ch] + A/2) / A.  The 2-D sum is exact: nothing is rounded between the horizontal and the vertical pass.
 * dst == src is allowed for fill only; a record with dst == src under pixelate or blur is skipped (other workgroups read src outside
 * their tile), as is, with its dst not written, a record with a null src or dst, a non-positive size, h > max_h or w > max_w.  A frame
 * with a bad prefix pair has no rows; it is still copied and its coasting tracks still apply.  For every frame not skipped the call
 * writes every byte of dst (in place: every byte that changes) and nothing outside it.  A tile no region meets is moved with 16-byte
 * accesses where src and dst allow the same ones, bytes at the ragged ends.  Device data is never trusted as a bound: age, id and the
 * box values of tracks are data, not indices.
 * Kernel shape: a tile is 64 x 16 pixels, four per thread.  Per tile the workgroup collects in LDS the regions whose bounding rectangle
 * (clipped to the frame) meets the tile -- the kept rows, then the stream's track slots, 256 candidates at a time, compacted by a
 * ballot prefix -- at 52 bytes per region (rectangle, the four G_q, kind), room for slots + max_tracks of them (max_tracks only with
 * tracks and coast > 0).  A tile with regions then stages, for pixelate, the rounded mean of every cell that meets the tile (4 bytes
 * per cell, at most ((63 / s) + 2) * ((15 / s) + 2) cells; each cell summed from src by a group of min(64, s*s rounded up to a power of
 * two) lanes, so a cell that straddles a tile seam is summed once by each tile it meets), and for blur the tile with its halo of r
 * pixels, clamped to the frame, (64 + 2r) * (16 + 2r) * c bytes, and its horizontal window sums as uint16, (16 + 2r) * 64 * c * 2 bytes:
 * 18432 + 24576 bytes at r = 16, c = 4.  At the limits (1024 + 256 regions, blur, r = 16, c = 4) that is 66560 + 43008 = 109568
 * bytes of the CU's 160 KiB; with 10 rows and 64 track slots, 3848 bytes of list.  There is no scratch buffer and there are no atomics.
 * Refused with DBX_ERR_ARG before anything is queued: batch < 0, c outside 1..4, max_h or max_w < 1, det_cols not 5 or 13, slots
 * outside 1..1024, det_rows < 0 (or below batch * slots in slot layout), method outside 0..2, shape outside 0..1, cell outside 2..32,
 * radius outside 1..16, grow outside 0..64, grow_pct outside 0..100, coast < 0, a NaN min_score, tracks given with stream0 < 0,
 * stream0 + batch > streams or max_tracks outside 1..256, a null frames / dets / keep / style, more than 2^24 - 1 tiles or 65535 frames
 * (one grid).  batch == 0: no-op.
 * dbx_redact_style is 40 bytes (color 0, method 4, shape 8, cell 12, radius 16, grow 20, grow_pct 24, coast 28, min_score 32).
 *
 * dbx_redact_host: the same region build, coverage test and value rules compiled for the host (no GPU needed), applied to ONE frame:
 * src and dst are host images [h][w][c]; rows float64 [n][det_cols] and keep, k row numbers of which the first min(k, n) are walked
 * (the device's clamp with slots = n); tracks, ntracks dbx_track records, or NULL.  It refuses what dbx_redact_batch refuses as far as
 * it applies, and also h or w < 1, n or k < 0, a null src or dst, null rows with n > 0, null keep with k > 0, ntracks outside 1..256
 * with tracks given, and dst == src under pixelate or blur. */
typedef struct dbx_redact_style {
    uint8_t color[4];      /* fill: channel ch of a covered pixel takes color[ch] */
    int32_t method;        /* 0 fill, 1 pixelate, 2 blur */
    int32_t shape;         /* 0 box, 1 quad (rows of 13 columns; others fall back to the box) */
    int32_t cell;          /* 2..32, pixelate's cell side */
    int32_t radius;        /* 1..16, blur's window is (2 radius + 1)^2 */
    int32_t grow;          /* 0..64 pixels added on every side */
    int32_t grow_pct;      /* 0..100 per cent of the region's size added on every side */
    int32_t coast;         /* >= 0: tracks of age 1..coast are redacted; 0: none */
    double  min_score;     /* rows with row[4] below it are skipped */
} dbx_redact_style;
int dbx_redact_batch(const dbx_overlay_frame* frames, int32_t batch, int32_t c, int32_t max_h, int32_t max_w, const double* dets,
                     int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix, int32_t slots,
                     const dbx_track* tracks, int32_t streams, int32_t stream0, int32_t max_tracks, const dbx_redact_style* style,
                     void* stream);
int dbx_redact_host(const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t c, const double* rows, int32_t det_cols, int32_t n,
                    const int32_t* keep, int32_t k, const dbx_track* tracks, int32_t ntracks, const dbx_redact_style* style);

/* ---- zones behind the tracker (no reference counterpart): a region-of-interest filter on the keep lists, counted line crossings and
 * region enter / exit events of the tracks, all on the device.  The semantics are this project's own, restated in plain integers by
 * tests/zones_ref.py ----
 * Coordinates: all geometry is in QUARTER PIXELS, int32 with |v| <= 2^20; every product is taken in int64 (a cross product of two
 * differences is at most 2^43 in magnitude for configured points, 2^47 with anchors).  A front end converts a user's float v with
 * int(floor(4 * v + 0.5)) and refuses non-finite values and values out of range.
 * Anchor of a box (x1, y1, x2, y2), float64: valid when all four values are finite with |v| < 2^20 (dbx_redact_batch's landmark rule).
 * ax = floor((x1 + x2) * 2.0 + 0.5); ay = floor((y1 + y2) * 2.0 + 0.5) for anchor = 0 (centre), ay = floor(y2 * 4.0 + 0.5) for anchor = 1
 * (bottom); evaluated in exactly this order, one IEEE operation per written operation, no contraction.
 * Configuration: dbx_zone_config [streams], a device table written from the host and never changed by a launch: per stream up to 8
 * directed lines A -> B (A != B), 8 count regions and 8 mask polygons, each mask marked include (role 0) or exclude (role 1); a region's
 * role is 0.  A polygon has 3..16 vertices in either orientation, may be concave and may intersect itself.
 * Point in polygon: even-odd.  Edge (xi, yi) -> (xj, yj), j = i + 1 mod n, counts when (yi > py) != (yj > py) and, with d = yj - yi,
 * l = (px - xi) * d, r = (xj - xi) * (py - yi): l < r if d > 0, else l > r.  Inside when the count is odd.  (Half-open: of an axis-aligned
 * rectangle the edges at the smaller x and the smaller y belong to it, the other two do not; a horizontal edge never counts.)
 * Side of a line: side(P) = cross(B - A, P - A) >= 0, cross(u, v) = ux * vy - uy * vx.
 * Crossing: the move P0 -> P1 crosses A -> B when side(P0) != side(P1) and, with t(Q) = cross(P1 - P0, Q - P0),
 * (t(A) >= 0) != (t(B) >= 0).  Forward (kind 0) when side goes false -> true, backward (kind 1) otherwise.  (A point ON the line has
 * side true, so landing on the line from the false side is the crossing and leaving it to the true side is none.)
 *
 * dbx_zone_filter_keep: ONE launch, a workgroup of 256 threads per frame; capturable.  It reads the rows and keep lists of the decoded-rows
 * description (both layouts, through the same reading rule as dbx_track_update_batch; frame b belongs to stream stream0 + b) and writes
 * keep_out, a buffer of the same layout and size (keep_out != keep).  With k the clamped count and E = min(rows of the frame, slots):
 * a stream without mask polygons has its k entries copied as they are; otherwise an entry stays when it names a row of the frame, the
 * row's anchor is valid, the anchor is inside at least one include polygon (or the stream has none) and inside no exclude polygon.  The
 * survivors keep their order; word 0 is the new count and the words behind the survivors up to position E are 0.  A frame of the packed
 * layout with a corrupt prefix pair has no list and nothing of keep_out is written for it (pairs that are each valid but overlap one
 * another give lists that overlap in keep_out as they do in keep: in bounds, their content unspecified).  stats: int32 [batch][2] = (k, survivors).
 * LDS: the stream's mask polygons, 1088 bytes, and 16 bytes of wave totals.
 *
 * dbx_zone_update_batch: ONE launch, a workgroup per frame, a thread per track slot; capturable.  It runs BEHIND dbx_track_update_batch
 * of the same frames, on the tracker's table and headers; frame f = headers[s].frame - 1.  Zone state: dbx_zone_state
 * [streams][max_tracks], 32 bytes: owner_id (-1 initially, the rest 0), has_prev, px, py, inside (bit r: region r), reserved.  For the
 * slots t of stream s in ascending order, K = tracks[s][t], Z = state[s][t], events in this order:
 *   1  owner left   Z.owner_id >= 0 and K.id != Z.owner_id (the slot is free or holds another id): for every bit r set in Z.inside,
 *                   ascending over all 8, an event of kind 4 ("ended inside") with the old owner's id, hits 0 and the stored (px, py);
 *                   exits[r] += 1, occupancy[r] -= 1.  Then Z = (-1, 0, 0, 0, 0).
 *   2  crossings    K.id >= 0 and K.hits >= min_hits (else the slot is done).  When K.id != Z.owner_id: owner_id = K.id, has_prev = 0,
 *                   inside = 0.  With a valid anchor P of K.box and has_prev: for every line l < n_lines, ascending, when (px, py) -> P
 *                   crosses it an event of kind 0 or 1 and forward[l] += 1 or backward[l] += 1.
 *   3  transitions  with a valid anchor: for every region r < n_regions, ascending, when "P is inside region r" differs from bit r of
 *                   inside an event of kind 2 (enter: enters[r] += 1, occupancy[r] += 1) or 3 (exit: exits[r] += 1, occupancy[r] -= 1)
 *                   and the bit flips; bits of regions not configured stay.  Then (px, py) = P, has_prev = 1.  With an invalid anchor:
 *                   no events, has_prev = 0, inside as it is.
 * A live slot with hits < min_hits leaves no zone state, so a track first seen inside a region enters it in the first frame it
 * qualifies.  A coasting track counts like any other: its box is the prediction.  An event is a dbx_zone_event, 32 bytes: stream,
 * track_id, kind, index (line or region), frame, hits (K.hits; 0 for kind 4), ax, ay (P; the stored point for kind 4).  The events of
 * frame b go to staged[b][0 .. staged_count[b] - 1], staged being dbx_zone_event [batch][max_tracks * 24] (per slot at most 8 ended
 * inside + 8 crossings + 8 transitions); staged and dbx_zone_append's events are 16-byte aligned.  line_counts: int64 [streams][8][2] = (forward, backward); region_counts:
 * int64 [streams][8][3] = (enters, exits, occupancy).  commit = 0 reads everything and writes NOTHING (state, counters, staged and
 * staged_count included): the dry mode of a graph's warm-up runs, as in dbx_track_gallery_update.  LDS: the stream's table, 2320 bytes,
 * 160 bytes of counter deltas and 16 bytes of wave totals; no scratch buffer beyond staged.
 *
 * dbx_zone_append: one small launch behind the update, dbx_track_append's pattern: the staged events of the call go to events[cursor...]
 * in frame order, then staging order; staged_count[b] is clamped to 0..max_tracks * 24.  state: device int64 [4] = {cursor, dropped,
 * total, reserved}; events past `capacity` are counted in dropped and not written.
 *
 * Robustness: nothing outside the buffers is read or written, whatever device data says: counts read from device memory (keep counts,
 * n_lines, n_regions, n_masks, a polygon's n, staged_count) are clamped before they bound a loop, table coordinates are clamped to
 * +-2^20 on the way to LDS, ids, hits and boxes are data.  A corrupt prefix pair gives an empty frame: its tracks coast and the zone
 * update still runs.  Refused with DBX_ERR_ARG before anything is queued: batch < 0, stream0 < 0 or stream0 + batch > streams, slots
 * outside 1..1024, det_cols not 5 or 13, det_rows < 0 (or below batch * slots in slot layout), max_tracks outside 1..256, min_hits < 1,
 * an anchor other than 0 / 1, capacity < 0, a null pointer (events only when capacity is 0), keep_out == keep.  batch == 0: no-op.
 *
 * dbx_zone_check_config validates a HOST copy of one stream's table: the three counts in 0..8 and, for the entries below them, a
 * polygon's n in 3..16, every coordinate within +-2^20, A != B, a region's role 0 and a mask's role 0 or 1.
 * dbx_zone_host runs the kernels' own geometry functions on the CPU (no GPU needed), n cases per call: op 0 / 1 the centre / bottom
 * anchor of boxes float64 [n][4] -> out int32 [n][3] = (valid, ax, ay); op 2 side of ints [n][6] = (ax, ay, bx, by, px, py) -> out [n]
 * = 0 / 1; op 3 crossing of ints [n][8] = (ax, ay, bx, by, x0, y0, x1, y1) -> out [n] = -1 none, 0 forward, 1 backward; op 4 point in
 * polygon of ints [n][35] = (px, py, n, xy[32]) -> out [n] = 0 / 1.
 *
 * Layouts: dbx_zone_line 16 bytes (ax 0, ay 4, bx 8, by 12); dbx_zone_poly 136 bytes (n 0, role 4, xy 8: x, y interleaved);
 * dbx_zone_config 2320 bytes (n_lines 0, n_regions 4, n_masks 8, reserved 12, lines 16, regions 144, masks 1232); dbx_zone_state 32
 * bytes (owner_id 0, has_prev 4, px 8, py 12, inside 16, reserved 20); dbx_zone_event 32 bytes (stream 0, track_id 4, kind 8, index 12,
 * frame 16, hits 20, ax 24, ay 28). */
typedef struct dbx_zone_line { int32_t ax, ay, bx, by; } dbx_zone_line;
typedef struct dbx_zone_poly {
    int32_t n;             /* 3..16 vertices */
    int32_t role;          /* masks: 0 include, 1 exclude; regions: 0 */
    int32_t xy[32];        /* x0, y0, x1, y1, ... in quarter pixels */
} dbx_zone_poly;
typedef struct dbx_zone_config {
    int32_t n_lines, n_regions, n_masks, reserved;
    dbx_zone_line lines[8];
    dbx_zone_poly regions[8];
    dbx_zone_poly masks[8];
} dbx_zone_config;
typedef struct dbx_zone_state {
    int32_t owner_id;      /* the track id the slot's zone state belongs to; -1 none */
    int32_t has_prev;      /* (px, py) is the anchor of the previous frame */
    int32_t px, py;
    int32_t inside;        /* bit r: inside region r */
    int32_t reserved[3];
} dbx_zone_state;
typedef struct dbx_zone_event {
    int32_t stream, track_id;
    int32_t kind;          /* 0 forward crossing, 1 backward crossing, 2 enter, 3 exit, 4 ended inside */
    int32_t index;         /* the line (kinds 0, 1) or the region */
    int32_t frame, hits, ax, ay;
} dbx_zone_event;
int dbx_zone_filter_keep(const double* dets, int32_t det_cols, int64_t det_rows, const int32_t* keep, const int32_t* prefix, int32_t batch,
                         int32_t slots, const dbx_zone_config* config, int32_t streams, int32_t stream0, int32_t anchor,
                         int32_t* keep_out, int32_t* stats, void* stream);
int dbx_zone_update_batch(const dbx_track* tracks, const int32_t* headers, const dbx_zone_config* config, dbx_zone_state* state,
                          int64_t* line_counts, int64_t* region_counts, int32_t batch, int32_t streams, int32_t stream0,
                          int32_t max_tracks, int32_t min_hits, int32_t anchor, dbx_zone_event* staged, int32_t* staged_count,
                          int32_t commit, void* stream);
int dbx_zone_append(const dbx_zone_event* staged, const int32_t* staged_count, int32_t batch, int32_t max_tracks, dbx_zone_event* events,
                    int64_t capacity, int64_t* state, void* stream);
int dbx_zone_check_config(const dbx_zone_config* config);
int dbx_zone_host(int32_t op, int64_t n, const double* boxes, const int32_t* ints, int32_t* out);

/* ---- batched pad + bicubic resize (pad_img + cv2.resize(..., INTER_CUBIC), DenseBox.py:1282-1340; the patch cutters' resize of a
 * cropped window) ----
 * One launch over njobs jobs.  A job reads a VIRTUAL source: the crop [cy0, cy0 + ch) x [cx0, cx0 + cw) of an interleaved uint8 image
 * [sh][sw][c] with pad_l / pad_t / pad_r / pad_b columns / rows of the constant pad_value around it -- what np.pad of the crop gives,
 * never materialised -- of vh x vw = (ch + pad_t + pad_b) x (cw + pad_l + pad_r) pixels, and writes its dh x dw resize as a contiguous
 * [dh][dw][c] block at byte offset dst_off of `dst` (64-bit; any alignment: whole 16-byte words of a row are stored as such, the
 * partial first / last word of a row as dwords, then bytes, and no byte outside the block is written).
 * Arithmetic: the generic C path of OpenCV's 8-bit INTER_CUBIC, restated.  Column dx: fx = (float)((dx + 0.5) * ((double)vw / dw) - 0.5),
 * sx = floor(fx), fx -= sx; float coefficients with A = -0.75 (c0 = ((A*(fx+1) - 5A)*(fx+1) + 8A)*(fx+1) - 4A, c1 = ((A+2)*fx - (A+3))*fx*fx + 1,
 * c2 the same in 1 - fx, c3 = 1 - c0 - c1 - c2), each rounded to int16 as saturate(rint(c * 2048)), no sum correction; taps sx-1 .. sx+2
 * clamped to [0, vw - 1] (replicate border of the virtual source).  Rows alike.  acc = sum of beta * alpha * pixel in int32
 * (|acc| <= 255 * (1.375 * 2048)^2 < 2^31); out = saturate_u8((acc + 2^21) >> 22).  Parity with an OpenCV build is unpinned.
 * Jobs may read different images of different sizes and write different sizes; all share the channel count c (1..4).  `jobs` is a
 * HOST array: the library copies its device records into `workspace` (device, dbx_resize_batch_workspace_bytes(njobs) bytes) on
 * `stream`, so the caller may reuse `jobs` when the call returns and must keep `workspace` until the launch has run.  Refused with
 * DBX_ERR_ARG before anything is queued: njobs < 0, c outside 1..4, a null pointer, a non-positive size, an image above 2^31 - 1
 * bytes, a crop outside its image, negative padding, a padded side above 2^30, pad_value outside 0..255, a negative dst_off, more
 * tiles than one grid holds (2^24 - 1 workgroups of 16 x 64 pixels).  njobs == 0: no-op.
 * Layout (72 bytes): src 0, sh 8, sw 12, cx0 16, cy0 20, cw 24, ch 28, pad_l 32, pad_t 36, pad_r 40, pad_b 44, pad_value 48, dh 52,
 * dw 56, (4 bytes of alignment padding,) dst_off 64. */
typedef struct dbx_resize_job {
    const uint8_t* src;                      /* device image [sh][sw][c] */
    int32_t sh, sw;
    int32_t cx0, cy0, cw, ch;                /* crop window inside the image */
    int32_t pad_l, pad_t, pad_r, pad_b;      /* constant padding around the crop */
    int32_t pad_value;                       /* 0..255 */
    int32_t dh, dw;                          /* destination size */
    int64_t dst_off;                         /* byte offset of this job's [dh][dw][c] output in dst */
} dbx_resize_job;
int64_t dbx_resize_batch_workspace_bytes(int32_t njobs);
int dbx_resize_cubic_batch_u8(const dbx_resize_job* jobs, int32_t njobs, int32_t c, uint8_t* dst, void* workspace, void* stream);

/* ---- NV12 frames in and out (no reference counterpart): what a video decoder hands out and an encoder takes, converted to and from
 * the interleaved uint8 RGB every other entry point reads, and resized straight from the NV12 surface.  The semantics are this project's
 * own, restated in NumPy by tests/nv12_ref.py ----
 * An NV12 frame of h x w pixels, h and w both even: a Y plane of h rows of pitch_y >= w bytes and a UV plane of h / 2 rows of
 * pitch_uv >= w bytes holding U0 V0 U1 V1 ...  Pixel (x, y) uses Y[y][x], U = UV[y >> 1][x & ~1] and V = UV[y >> 1][(x & ~1) + 1]:
 * chroma is REPLICATED over its 2 x 2 block.  There is NO chroma interpolation, in either direction.  The RGB image is interleaved
 * [h][pitch_rgb bytes] with pitch_rgb >= 3 * w.  Every pointer and every pitch may have any byte alignment.
 * dbx_nv12_params: standard 601 or 709 (Kr, Kb = 0.299, 0.114 or 0.2126, 0.0722; Kg = 1 - Kr - Kb), range 0 limited (Y 16..235, chroma
 * 16..240) or 1 full, order 0 RGB or 1 BGR (the byte order of a pixel of the interleaved image; the engine's uint8 input is RGB).
 * All arithmetic is 14-bit integer: every coefficient is rint(c * 16384) of the float64 constant, and >> is the arithmetic shift (floor).
 * To RGB: ys, cs, yo = 255/219, 255/224, 16 (limited) or 1, 1, 0 (full); C = Y - yo, D = U - 128, E = V - 128;
 *   R = clip8((ky*C + rv*E + 8192) >> 14), G = clip8((ky*C + gu*D + gv*E + 8192) >> 14), B = clip8((ky*C + bu*D + 8192) >> 14)
 *   with ky = ys, rv = cs*2(1-Kr), gu = -cs*2Kb(1-Kb)/Kg, gv = -cs*2Kr(1-Kr)/Kg, bu = cs*2(1-Kb): the DBX_NV12_*_TO_RGB integers below.
 * From RGB: ys', cs' = 219/255, 224/255 (limited) or 1, 1 (full).  Per pixel Y = clip8(((yr*R + yg*G + yb*B + 8192) >> 14) + yo) with
 *   (yr, yg, yb) = ys' * (Kr, Kg, Kb).  Per 2 x 2 block, with the sums Rs, Gs, Bs of its four pixels (0..1020):
 *   U = clip8(((ur*Rs + ug*Gs + ub*Bs + 32768) >> 16) + 128), V = clip8(((vr*Rs + vg*Gs + vb*Bs + 32768) >> 16) + 128) with
 *   (ur, ug, ub) = cs' * (-Kr, -Kg, 1-Kb) / (2(1-Kb)) and (vr, vg, vb) = cs' * (1-Kr, -Kg, -Kb) / (2(1-Kr)): the DBX_NV12_*_FROM_RGB
 *   integers below, in the order yr, yg, yb, ur, ug, ub, vr, vg, vb.  The rounded chroma rows sum to exactly 0 in all four variants, so
 *   grey gives U = V = 128; the luma rows sum to 14071 (limited) or 16384 (full).
 * Each result is within 1 of the float64 formula rounded to nearest.  The round trip is NOT the identity: chroma is averaged over 2 x 2
 * blocks on the way out and replicated on the way back, limited range has fewer than 256 levels, and both directions round.
 *
 * dbx_nv12_to_rgb_batch / dbx_rgb_to_nv12_batch: ONE launch over a DEVICE table of `batch` dbx_nv12_frame records, a workgroup of 256
 * threads per 128 x 16 tile on a grid of (the tiles of a max_h x max_w frame, batch); nothing is copied from the host and nothing
 * synchronises.  to_rgb reads y and uv and writes rgb, from_rgb reads rgb and writes y and uv; for every frame not skipped every byte
 * of the w (3 * w) bytes of every output row is written and nothing else: not the pitch gap behind a row, nothing outside the planes.
 * A record is skipped, with nothing of it written, when a pointer is null, h or w is non-positive or odd, h > max_h or w > max_w, or
 * a pitch is below its row (pitch_y < w, pitch_uv < w, pitch_rgb < 3 * w).  Device data is never trusted as a bound beyond that.
 * Kernel shape: half of the workgroup's lanes own 8 x 2 pixels each -- four whole 2 x 2 blocks, so each UV pair is loaded (written)
 * once -- and move the Y and UV bytes as one 8-byte word per row where the address allows, else as two dwords, else as bytes (also for
 * the ragged last lane of a row).  The RGB side is staged in LDS, every tile row at the offset its global address has inside a 16-byte
 * word, and moved by 16 lanes per row as aligned 16-byte words, with a dword and then a byte fall-back for the partial first and last
 * word of a row (the store of the resize tile, csrc/resize_tile.hpp).  4.5 bytes move per pixel in either direction; no scratch, no atomics.
 * Refused with DBX_ERR_ARG before anything is queued: batch < 0, max_h or max_w < 1, a null frames or params, standard not 601 or 709,
 * range or order outside 0..1, more than 2^24 - 1 tiles or 65535 frames (one grid).  batch == 0: no-op.
 * dbx_nv12_frame is 48 bytes (y 0, uv 8, rgb 16, h 24, w 28, pitch_y 32, pitch_uv 36, pitch_rgb 40, reserved 44); dbx_nv12_params is
 * 16 bytes (standard 0, range 4, order 8, reserved 12).
 *
 * dbx_nv12_host: the same pixel functions compiled for the host (no GPU needed) on ONE frame whose pointers are host memory;
 * direction 0 converts to RGB, 1 from RGB.  It REFUSES what the launches skip (a null pointer, a non-positive or odd size, a pitch
 * below its row), a null frame or params, a bad enum and a direction outside 0..1.
 *
 * dbx_resize_cubic_batch_nv12: dbx_resize_cubic_batch_u8 with c = 3 whose virtual source is the CONVERTED frame, never materialised: a
 * tap inside the crop is fetched as Y, U, V and converted, once per tap (16 conversions per output pixel, not 48); a padded tap
 * contributes pad_value in all three channels.  The result is bit for bit dbx_resize_cubic_batch_u8 on dbx_nv12_to_rgb_batch's output.
 * dbx_resize_job_nv12 is dbx_resize_job with y, uv, pitch_y, pitch_uv in the place of src; sh and sw are even; the crop window may start
 * at odd coordinates and have odd sizes, because chroma is indexed by absolute source coordinates.  The workspace
 * (dbx_resize_batch_nv12_workspace_bytes(njobs) device bytes) and the life times are dbx_resize_cubic_batch_u8's.  Refused with
 * DBX_ERR_ARG before anything is queued: what dbx_resize_cubic_batch_u8 refuses (with both planes in the place of src and pitch_y * sh
 * in the place of the image's bytes), odd or non-positive sh or sw, pitch_y < sw, pitch_uv < sw, and bad params.
 * Layout (88 bytes): y 0, uv 8, pitch_y 16, pitch_uv 20, sh 24, sw 28, cx0 32, cy0 36, cw 40, ch 44, pad_l 48, pad_t 52, pad_r 56,
 * pad_b 60, pad_value 64, dh 68, dw 72, (4 bytes of alignment padding,) dst_off 80. */
#define DBX_NV12_601_LIMITED_TO_RGB 19077, 26149, -6419, -13320, 33050
#define DBX_NV12_601_FULL_TO_RGB 16384, 22970, -5638, -11700, 29032
#define DBX_NV12_709_LIMITED_TO_RGB 19077, 29372, -3494, -8731, 34610
#define DBX_NV12_709_FULL_TO_RGB 16384, 25802, -3069, -7670, 30402
#define DBX_NV12_601_LIMITED_FROM_RGB 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170
#define DBX_NV12_601_FULL_FROM_RGB 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332
#define DBX_NV12_709_LIMITED_FROM_RGB 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660
#define DBX_NV12_709_FULL_FROM_RGB 3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751
typedef struct dbx_nv12_frame {
    uint8_t* y;                              /* [h][pitch_y] */
    uint8_t* uv;                             /* [h / 2][pitch_uv], U0 V0 U1 V1 ... */
    uint8_t* rgb;                            /* [h][pitch_rgb], interleaved */
    int32_t h, w;                            /* both even */
    int32_t pitch_y, pitch_uv, pitch_rgb;    /* bytes per row: >= w, >= w, >= 3 * w */
    int32_t reserved;
} dbx_nv12_frame;
typedef struct dbx_nv12_params {
    int32_t standard;                        /* 601 or 709 */
    int32_t range;                           /* 0 limited, 1 full */
    int32_t order;                           /* 0 RGB, 1 BGR */
    int32_t reserved;
} dbx_nv12_params;
typedef struct dbx_resize_job_nv12 {
    const uint8_t* y;                        /* device Y plane [sh][pitch_y] */
    const uint8_t* uv;                       /* device UV plane [sh / 2][pitch_uv] */
    int32_t pitch_y, pitch_uv;
    int32_t sh, sw;                          /* both even */
    int32_t cx0, cy0, cw, ch;                /* crop window inside the frame; may be odd */
    int32_t pad_l, pad_t, pad_r, pad_b;      /* constant padding around the crop */
    int32_t pad_value;                       /* 0..255, in all three channels */
    int32_t dh, dw;                          /* destination size */
    int64_t dst_off;                         /* byte offset of this job's [dh][dw][3] output in dst */
} dbx_resize_job_nv12;
int dbx_nv12_to_rgb_batch(const dbx_nv12_frame* frames, int32_t batch, int32_t max_h, int32_t max_w, const dbx_nv12_params* params,
                          void* stream);
int dbx_rgb_to_nv12_batch(const dbx_nv12_frame* frames, int32_t batch, int32_t max_h, int32_t max_w, const dbx_nv12_params* params,
                          void* stream);
int dbx_nv12_host(const dbx_nv12_frame* frame, const dbx_nv12_params* params, int32_t direction);
int64_t dbx_resize_batch_nv12_workspace_bytes(int32_t njobs);
int dbx_resize_cubic_batch_nv12(const dbx_resize_job_nv12* jobs, int32_t njobs, const dbx_nv12_params* params, uint8_t* dst,
                                void* workspace, void* stream);

/* ---- training patch sampling (gen_pos_patch, process_plate.py:167-352, with format_4_vertices :109 and bbox_from_vertices :1247; the
 * negative path of gen_pure_neg_patches :711-749 with intersect_small :639-666) ----
 * Two launches and no host read between them: dbx_patch_plan (ONE workgroup) decides M candidates, gives the accepted ones their
 * output slots in candidate order and writes a job record + a label row per slot; dbx_patch_cut (n * 60 workgroups, fixed by n alone)
 * runs the batched resize's tile body on those records into patches uint8 [n][240][240][c].  Both can be captured into a hipGraph.
 *
 * Tables (device): frames = n_frames dbx_crop_frame records; plates int32 [n_plates][9] = (frame, x0, y0, x1, y1, x2, y2, x3, y3), the
 * four vertices in annotation order, rows sorted by frame; plate0 int32 [n_frames + 1], plate0[f] .. plate0[f + 1] the rows of frame f.
 *
 * Candidate i is (kind, index, d0, d1): kind 0 = positive (index: a plates row; d0, d1: the two uniform(-1, 1) values), kind 1 =
 * negative (index: a frame; d0, d1: the integer centre x, y as doubles).
 *   injected mode (io->cand and io->draws both non-NULL): read from cand int32 [M][2] and draws float64 [M][2].
 *   device mode (both NULL): made from the hash h(seed, counter, i, j) of draw number j = 0..3 below, k = h >> 11 (53 bits):
 *     j = 0  kind: negative when k * 2^-53 < neg_frac (with n_plates == 0 every candidate is negative, with neg_frac == 0 none is)
 *     j = 1  index: k mod n_plates (positive) or k mod n_frames (negative)
 *     j = 2, 3  positive: d = -1.0 + 2.0 * (k * 2^-53), the value set of Python's random.uniform(-1, 1);
 *               negative: d0 = 120 + k mod (W - 240), d1 = 120 + k mod (H - 240) of the drawn frame (0, 0 when status 5)
 *     state = device int64 [2] = (seed, counter); the launch's last act is counter += 1, so a replay of a captured launch draws anew.
 *   Both modes write the candidates they used to cand_out / draws_out.
 * The hash (unsigned 64-bit arithmetic, wrapping):
 *     mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *     h = mix(mix(seed + 0x9E3779B97F4A7C15 * (counter + 1)) + 0xD1B54A32D192ED03 * (i + 1) + 0x8CB92BA72F3D8DD7 * (j + 1))
 *
 * Geometry of a positive in a W x H frame (float64, the reference's order of operations, no contraction; I(x) = (int)(x + 0.5),
 * truncation toward zero, saturated to +-10^9 where Python would go on):
 *   status 4 when the frame record has a null src, a non-positive size or more than 2^31 - 1 bytes, or a vertex has x outside
 *     0 .. W - 1 or y outside 0 .. H - 1 -- refused before any geometry (the reference would go on with negative slice indices).
 *   d0 or d1 not finite (|d| > 10^100, injected mode only): status 2.
 *   format_4_vertices: a STABLE sort of the four on x; the first two are the left pair, the others IN ANNOTATION ORDER the right pair
 *     (membership by value); of each pair the first in a stable sort on y is "up".  Any two vertices equal by value make the reference
 *     raise IndexError: status 2.
 *   bbox = (min(lu.x, ld.x), max(ru.x, rd.x), min(lu.y, ru.y), max(ld.y, rd.y)); cx = I((x_min + x_max) * 0.5), cy alike;
 *   pw = 4.0 * (x_max - x_min), ph alike; org = (cx - pw * 0.5 - d0 * offset_radius, cy - ph * 0.5 - d1 * offset_radius);
 *   end = org + (pw, ph); then :208-222: if org.x < 0 or org.y < 0: each negative org becomes 0 and pw, ph = end - org; if
 *   end.x >= W or end.y >= H: end.x = W - 1 where end.x >= W, end.y = H - 1 where end.y >= H, and pw, ph = end - org.
 *   pw == 0 or ph == 0 (ZeroDivisionError in the reference): status 2.
 *   label = I(((v - org) / (pw, ph)) * 240.0) for bbox left-up, bbox right-down, lu, ru, rd, ld: the 12 integers of the file name.
 *   The rule :274-277, literally, with the SOURCE frame's W and H: rejected (status 1) when lu.x < 8 or lu.y < 8 or ru.x > W - 8 or
 *     ru.y < 8 or rd.x > W - 8 or rd.y > H - 8 or ld.x < 8 or ld.y > H - 8.
 *   slice = I(org) : I(end) on both axes; x1 <= x0 or y1 <= y0: status 3 (the reference returns an empty patch).  A patch that passes
 *     the rule has end > 0, so no index is negative and the slice is the window as it stands.
 * A negative in frame f: status 4 for an unusable frame record; status 5 when W < 241 or H < 241 or (injected) the centre is not an
 * integer pair with 120 <= cx < W - 120, 120 <= cy < H - 120; status 2 when ANY plate of the frame has two equal vertices (every plate is
 * formatted before the test runs); then intersect_small over the frame's plates in order, with a plate's sorted lu, rd:
 * iw = min(rd.x, cx + 120) - max(lu.x, cx - 120), ih alike; iw < 0 or ih < 0: accepted at once; iw * ih > th: status 6; all plates passed (or none): accepted.  The window is [cx - 120, cx + 120) x [cy - 120,
 * cy + 120) at scale 1, which the 11-bit coefficients make an exact copy; the label row is all zero.
 * An index outside its table (which dbx_patch_check_tables refuses on the host) is never followed: status 2.
 *
 * status: 0 accepted, 1 landmark rule, 2 degenerate, 3 empty slice, 4 vertex outside its frame, 5 negative: no 240 x 240 window,
 * 6 negative: overlaps a plate, 7 accepted but beyond the capacity n.
 * Slots: an exclusive scan of the accept flags in candidate order; slot[i] = that rank for an accepted candidate (status 0: < n, status 7:
 * >= n), -1 otherwise.  count = min(accepted, n).  Slot s < count gets jobs[s], labels[s] (int32 [12]; all zero for a negative), bbox[s] =
 * labels[s][0..3] / 4, vertices[s] = labels[s][4..11] / 4 and label[s] = 1 (0 for a negative) as float32 -- what DenseBoxDataset reads
 * from the file name.  Rows at or past count are not written.  tally[k] = candidates with status k.
 * dbx_patch_job (96 bytes, the resize kernel's device record): src 0, dst 8 (unused: 0), scale_x 16, scale_y 24 (cw / 240.0, ch / 240.0),
 * row_bytes 32 (sw * c), cx0 36, cy0 40, cw 44, ch 48, pad_l 52, pad_t 56 (0), vw 60, vh 64 (= cw, ch), dh 68, dw 72 (240), pad_value 76
 * (0), tiles_x 80 (4), frame 84, kind 88, reserved 92. */
#define DBX_PATCH_SIDE 240
#define DBX_PATCH_MAX_CAND 4096
#define DBX_PATCH_NSTATUS 8
typedef struct dbx_patch_job {
    const uint8_t* src;
    uint8_t* dst;
    double scale_x, scale_y;
    int32_t row_bytes;
    int32_t cx0, cy0, cw, ch, pad_l, pad_t, vw, vh, dh, dw, pad_value, tiles_x;
    int32_t frame, kind, reserved;
} dbx_patch_job;
/* one candidate's geometry (72 bytes): status 0, x0 4, y0 8, x1 12, y1 16 (the slice; zeros unless status is 0 or 3), labels 20, reserved 68 */
typedef struct dbx_patch_geom {
    int32_t status;
    int32_t x0, y0, x1, y1;
    int32_t labels[12];
    int32_t reserved;
} dbx_patch_geom;
/* device pointers of dbx_patch_plan (136 bytes: 17 pointers in this order) */
typedef struct dbx_patch_plan_io {
    const dbx_crop_frame* frames;
    const int32_t* plates;       /* [n_plates][9]; may be NULL when n_plates == 0 */
    const int32_t* plate0;       /* [n_frames + 1] */
    const int32_t* cand;         /* [M][2] (kind, index), or NULL: device mode */
    const double* draws;         /* [M][2], or NULL: device mode */
    int64_t* state;              /* [2] (seed, counter); needed in device mode only */
    dbx_patch_job* jobs;         /* [n] */
    int32_t* labels;             /* [n][12] */
    float* bbox;                 /* [n][4] */
    float* vertices;             /* [n][8] */
    float* label;                /* [n][1] */
    int32_t* count;              /* [1] */
    int32_t* tally;              /* [DBX_PATCH_NSTATUS] */
    int32_t* status;             /* [M] */
    int32_t* slot;               /* [M] */
    int32_t* cand_out;           /* [M][2] */
    double* draws_out;           /* [M][2] */
} dbx_patch_plan_io;
/* Refused with DBX_ERR_ARG before anything is queued: a null io or a null pointer in it (cand and draws: both or neither; state may be NULL
 * in injected mode; plates may be NULL when n_plates == 0; status, slot, cand_out, draws_out may be NULL when M == 0), n_frames < 1,
 * n_plates < 0, c outside 1..4, M outside 0..4096, n < 1, neg_frac not in [0, 1], offset_radius not finite or negative, th < 0.
 * M == 0: count = 0, a zero tally, and (device mode) the counter still advances. */
int dbx_patch_plan(const dbx_patch_plan_io* io, int32_t n_frames, int32_t n_plates, int32_t c, int32_t M, int32_t n, double neg_frac,
                   double offset_radius, int32_t th, void* stream);
/* jobs / count as dbx_patch_plan left them; patches device uint8 [n][240][240][c] at any byte alignment.  Slot s < min(count, n) is bit for
 * bit dbx_resize_cubic_batch_u8 of its window to 240 x 240; slots at or past count are not written.  Refused: a null pointer, n < 1 or
 * above 2^24 / 60, c outside 1..4. */
int dbx_patch_cut(const dbx_patch_job* jobs, const int32_t* count, int32_t n, int32_t c, uint8_t* patches, void* stream);
/* The plan's geometry of ONE candidate on the host (the same __host__ __device__ function the kernel runs), for a CPU check.  kind 0:
 * verts = the plate's 8 integers, n_verts = 1; kind 1: verts = the 8 integers of each of the frame's n_verts plates.  Refused: a null
 * pointer, kind outside 0..1, n_verts < 0 (or != 1 for kind 0), W or H < 1, th < 0. */
int dbx_patch_plan_host(int32_t kind, int32_t W, int32_t H, const int32_t* verts, int32_t n_verts, double d0, double d1,
                        double offset_radius, int32_t th, dbx_patch_geom* out);
/* out[(r * 4 + j)] = h(seed, counter, i0 + r, j) for r < count, j < 4 (the raw 64-bit hash).  Refused: a null out, count < 0, i0 < 0. */
int dbx_patch_draw(int64_t seed, int64_t counter, int32_t i0, int32_t count, uint64_t* out);
/* Host check of host copies of the tables, to be run before they are uploaded.  Refused with DBX_ERR_ARG: a null plate0, n_frames < 1,
 * n_plates < 0, a plates row whose frame is outside 0 .. n_frames - 1 or below the row before it (not sorted by frame), a plate0 that is
 * not the row prefix of those frames, and -- when cand is not NULL -- M outside 0..4096, a kind outside 0..1, a positive's index outside
 * 0 .. n_plates - 1, a negative's index outside 0 .. n_frames - 1. */
int dbx_patch_check_tables(const int32_t* plates, int32_t n_plates, const int32_t* plate0, int32_t n_frames, const int32_t* cand, int32_t M);

/* ---- training patch augmentation (this project's own semantics: the reference has none; tests/aug_ref.py restates them in NumPy) ----
 * Two launches after dbx_patch_cut and no host read: dbx_patch_aug_plan (ONE workgroup) decides a parameter record per slot and writes
 * the labels that go with it; dbx_patch_augment (n * 15 workgroups, fixed by n alone) makes the augmented patches, out of place.  All
 * pixel arithmetic is integer, every shift is arithmetic (a floor), clamp is to 0..255: the kernel equals the restatement bit for bit.
 *
 * dbx_patch_aug (64 bytes, 16 int32): flags 0 (bit 0: flip applied, bit 1: flip refused), blur 4 (0 none, 1 binomial 3 x 3, 2 binomial
 * 5 x 5, 3 horizontal box), box_len 8 (odd, 3..9; read by blur 3 only), sat 12 (Q8, 256 = identity), contrast 16 (Q8), brightness 20
 * (-255..255), curve 24 (a row of the bank, -1 = none), noise_amp 28 (Q8, 0 = none), key_lo 32, key_hi 36 (the low and the high half of
 * the 64-bit noise key), gain 40 (3 x Q8, one per colour channel), reserved 52 (3 x 0).
 * What a kernel reads of a record ("sanitised", the same function on host and device): flags & 3; a blur outside 0..3, or blur 3 with a
 * box_len that is even or outside 3..9, is blur 0; sat, contrast, gain and noise_amp are clamped to 0..65535, brightness to -255..255; a
 * curve outside 0 .. G - 1 is -1 (no kernel follows it); reserved is 0.  The records written out are the sanitised ones.
 *
 * A pixel (x, y) of a patch with c channels; the colour channels are the first min(c, 3), a fourth channel is flipped and blurred and
 * otherwise copied.  In this order:
 *   1. flip: with bit 0 the image is mirrored, I'(x, y) = I(239 - x, y).
 *   2. blur of the (mirrored) image, edges replicated (coordinates clamped to 0..239):
 *        blur 1: weights outer([1, 2, 1]), v = (sum + 8) >> 4;  blur 2: outer([1, 4, 6, 4, 1]), v = (sum + 128) >> 8 -- one rounding;
 *        blur 3: the box_len pixels of the row centred on x, v = (2 * sum + L) / (2 * L) in integer division.
 *   3. saturation, when c >= 3: Y = (v0 + 2 * v1 + v2 + 2) >> 2 (the gallery's luma weights, free of the channel order);
 *        v_k = clamp(Y + (((v_k - Y) * sat + 128) >> 8)).
 *   4. tone, per colour channel k: g = clamp((v * gain_k + 128) >> 8); t = clamp((((g - 128) * contrast + 128) >> 8) + 128 + brightness);
 *        with curve >= 0: t = curves[curve][t].  (The kernel composes a 256-entry table per colour channel.)
 *   5. noise, when noise_amp > 0: h = mix(key + 0x9E3779B97F4A7C15 * (y * 240 + x + 1)) with the sampler's mix and unsigned 64-bit
 *        wrapping, (x, y) the OUTPUT pixel; t_k = byte(h, 2k) + byte(h, 2k + 1) - 255 with byte(h, j) = (h >> 8j) & 255;
 *        d = t_k * noise_amp; the term is (d + 128) >> 8 for d >= 0 and -((-d + 128) >> 8) for d < 0 (half away from zero on both
 *        sides: a plain (d + 128) >> 8 rounds every half upward and has a mean of up to +1/4); v_k = clamp(v_k + term).
 * curves: device uint8 [G][256], made on the host (no pow on the device); may be NULL when G == 0.
 *
 * Labels.  labels_in int32 [n][12] = (bx0, by0, bx1, by1, lu, ru, rd, ld) as dbx_patch_plan wrote them; a row of twelve zeros is a
 * negative.  Without a flip the row is copied.  A flip of a positive: bx0' = 239 - bx1, bx1' = 239 - bx0, lu' = (239 - ru.x, ru.y),
 * ru' = (239 - lu.x, lu.y), rd' = (239 - ld.x, ld.y), ld' = (239 - rd.x, rd.y), every y as it was.  The plan's labels may be 240 on the
 * right edge: a positive with any of its six x values outside 0..239 is NOT flipped, pixels included; bit 0 is cleared and bit 1 set.  A
 * negative flips its pixels and keeps its zero row.  bbox = labels[0..3] / 4, vertices = labels[4..11] / 4 and label = 1 (0 for a
 * negative) as float32, exactly as dbx_patch_plan writes them.  Rows at or past min(count, n) are not written.
 *
 * Parameters.
 *   injected mode (io->params_in non-NULL): slot s reads params_in[s]; flags bit 0 asks for the flip, bit 1 is ignored.
 *   device mode (params_in NULL): from h(seed, counter, s, j) of the sampler's hash with a FIXED draw number j per field, k = h >> 11; "on
 *   with probability p" is k * 2^-53 < p; a range is lo + k mod (hi - lo + 1):
 *     j = 0 flip on (p_flip);  1 blur on (p_blur);  2 blur kind: w = k mod (kind_w[0] + kind_w[1] + kind_w[2]), kind 1 when w < kind_w[0],
 *     2 when w < kind_w[0] + kind_w[1], else 3;  3 box_len = box_lo + 2 * (k mod ((box_hi - box_lo) / 2 + 1));  4 sat;  5 contrast;
 *     6 brightness;  7 curve on (p_curve);  8 curve = curve_lo + k mod (curve_hi - curve_lo + 1);  9 noise on (p_noise);  10 noise_amp;
 *     11 the key (the whole hash);  12, 13, 14 gain[0..2].
 *   An op that is off writes its neutral value (blur 0, curve -1, noise_amp 0); box_len and the key are always the drawn ones.
 *   state = device int64 [2] = (seed, counter), the augmenter's own; the launch's last act is counter += 1, so a replay draws anew.
 *   Both modes write the records they used to io->params.
 * dbx_patch_aug_cfg (112 bytes): p_flip 0, p_blur 8, p_curve 16, p_noise 24 (double); kind_w 32 (3 x int32); box_lo 44, box_hi 48; sat_lo
 * 52, sat_hi 56; contrast_lo 60, contrast_hi 64; brightness_lo 68, brightness_hi 72; gain_lo 76, gain_hi 80; noise_lo 84, noise_hi 88;
 * curve_lo 92, curve_hi 96; G 100 (rows of the bank); reserved 104 (2 x 0). */
typedef struct dbx_patch_aug {
    int32_t flags, blur, box_len, sat, contrast, brightness, curve, noise_amp;
    int32_t key_lo, key_hi;
    int32_t gain[3];
    int32_t reserved[3];
} dbx_patch_aug;
typedef struct dbx_patch_aug_cfg {
    double p_flip, p_blur, p_curve, p_noise;
    int32_t kind_w[3];
    int32_t box_lo, box_hi, sat_lo, sat_hi, contrast_lo, contrast_hi, brightness_lo, brightness_hi, gain_lo, gain_hi, noise_lo, noise_hi;
    int32_t curve_lo, curve_hi, G;
    int32_t reserved[2];
} dbx_patch_aug_cfg;
/* device pointers of dbx_patch_aug_plan (72 bytes: 9 pointers in this order) */
typedef struct dbx_patch_aug_io {
    const int32_t* labels_in;          /* [n][12] */
    const int32_t* count;              /* [1] */
    const dbx_patch_aug* params_in;    /* [n], or NULL: device mode */
    int64_t* state;                    /* [2] (seed, counter); needed in device mode only */
    dbx_patch_aug* params;             /* [n] */
    int32_t* labels;                   /* [n][12] */
    float* bbox;                       /* [n][4] */
    float* vertices;                   /* [n][8] */
    float* label;                      /* [n][1] */
} dbx_patch_aug_io;
/* cfg is a HOST struct, needed in both modes (injected mode reads G alone).  Refused with DBX_ERR_ARG before anything is queued: a null
 * io, cfg or pointer (params_in may be NULL: device mode, which needs state), n outside 1..4096, and a cfg with: a p outside [0, 1], G
 * outside 0..65536, a kind weight outside 0..2^20 or -- with p_blur > 0 -- none positive, a box length that is even or outside 3..9, a range
 * with lo > hi, sat / contrast / gain / noise outside 0..65535, brightness outside -255..255, with p_curve > 0 a curve index range that
 * leaves the bank (0 <= curve_lo <= curve_hi < G). */
int dbx_patch_aug_plan(const dbx_patch_aug_io* io, const dbx_patch_aug_cfg* cfg, int32_t n, void* stream);
/* patches, out: device uint8 [n][240][240][c] at any byte address; params / count as dbx_patch_aug_plan left them (or any records: they
 * are sanitised).  Slot s < min(count, n) is written, every other byte of out is left alone.  Out of place only: a blurred band reads its
 * neighbours' rows.  Refused: a null pointer (curves may be NULL when G == 0), c outside 1..4, n outside 1..4096, G outside 0..65536,
 * patches and out overlapping. */
int dbx_patch_augment(const uint8_t* patches, const dbx_patch_aug* params, const int32_t* count, const uint8_t* curves, int32_t G,
                      int32_t n, int32_t c, uint8_t* out, void* stream);
/* dbx_patch_aug_plan on the host (the same __host__ __device__ functions) for slots 0 .. count - 1, count in 0..4096: params_in NULL
 * derives from (seed, counter).  Refusals as for dbx_patch_aug_plan. */
int dbx_patch_aug_params_host(const dbx_patch_aug_cfg* cfg, int64_t seed, int64_t counter, const dbx_patch_aug* params_in,
                              const int32_t* labels_in, int32_t count, dbx_patch_aug* params, int32_t* labels, float* bbox,
                              float* vertices, float* label);
/* dbx_patch_augment of ONE patch [240][240][c] on the host.  Refusals as for dbx_patch_augment. */
int dbx_patch_augment_host(const uint8_t* patch, const dbx_patch_aug* rec, const uint8_t* curves, int32_t G, int32_t c, uint8_t* out);

/* ---- training patch warp (this project's own semantics: the reference has no augmentation; tests/warp_aug_ref.py restates them) ----
 * The geometric half of the augmenter: rotation, scale, aspect, shear, translation and keystone of a cut patch, as ONE perspective
 * map per slot.  Two launches between dbx_patch_cut and dbx_patch_aug_plan and no host read: dbx_patch_warp_plan (ONE workgroup) decides
 * a record, the label row and the two 3 x 3 matrices of every slot; dbx_patch_warp (n * 15 workgroups, fixed by n alone) makes the
 * pixels, out of place.  fp contraction is off in the whole file, as for the rectification: host and device round alike.
 *
 * Quad and matrices.  A warp is given by a quad: eight int32 in 1/16 pixel, the places in the OUTPUT patch where the input patch's
 * corner pixel centres (0,0), (239,0), (239,239), (0,239) land, in that order; the identity quad is (0,0, 3824,0, 3824,3824, 0,3824).
 * fwd = M = the 8 x 8 solve of dbx_perspective_matrix on (square, quad / 16.0) in double (the division is exact); inv = the cofactor
 * inverse dbx_warp_perspective_u8 takes of M.
 *
 * Pixels.  Output pixel (x, y) of a warped slot is dbx_warp_perspective_u8's arithmetic on the 240 x 240 input patch with inv: the
 * float64 inverse map, cvRound to 1/32 pixel, 15-bit bilinear weights, (sum + 2^14) >> 15.  border 0 (constant): a neighbour outside the
 * patch contributes byte ch of fill (one byte per channel, channel ch in bits 8 ch .. 8 ch + 7); with fill 0 this is exactly
 * dbx_warp_perspective_u8.  border 1 (replicate): the four neighbour coordinates are clamped to 0..239.  A slot whose warp is not
 * applied (bit 0 of the written record clear) is a copy of its input.
 *
 * Labels.  labels_in int32 [n][12] as dbx_patch_plan writes them (box, lu, ru, rd, ld); twelve zeros are a negative, which keeps its
 * zero row and has its pixels warped.  A positive: each vertex (vx, vy) goes through M in float64, left to right:
 *   W = m6 * vx + m7 * vy + m8;  x' = I((m0 * vx + m1 * vy + m2) / W);  y' = I((m3 * vx + m4 * vy + m5) / W);  I(v) = v + 0.5 truncated
 *   toward zero;  the box is rebuilt as the plan builds it: bx0 = min(lu.x, ld.x), bx1 = max(ru.x, rd.x), by0 = min(lu.y, ru.y),
 *   by1 = max(ld.y, rd.y).  bbox = labels[0..3] / 4, vertices = labels[4..11] / 4, label = 1 (0 for a negative) as float32.
 * Refused by rule (a positive only): any W not finite or not > 0; any new vertex coordinate outside margin .. 239 - margin (a value
 * that is not finite counts as outside); bx1 <= bx0 or by1 <= by0.  A refused positive copies its pixels and its label row; bit 0 is
 * cleared and bit 1 set.
 * Degenerate (any slot that asks for the warp): the solve or the inverse fails (a pivot at or below 2^-52, a zero determinant), or any
 * of the 18 matrix entries is not finite.  A degenerate slot copies; bit 0 is cleared and bit 2 set.  Degeneracy is decided before the
 * label rule.  fwd and inv of every slot that copies are the exact identity.
 *
 * dbx_patch_warp_rec (64 bytes, 16 int32): flags 0 (bit 0: warp applied, bit 1: refused by the label rule, bit 2: degenerate), border 4
 * (0 constant, 1 replicate), fill 8, rot 12 (a row of the bank), quad 16 (8 x int32), scale 48 (Q8), aspect 52 (Q8), shear 56 (Q8, signed),
 * reserved 60 (0).  What a kernel reads of a record ("sanitised", the same function on host and device): flags & 1; a border outside
 * 0..1 is 0; quad entries are clamped to +-2^20; reserved is 0.  rot, scale, aspect and shear are carried, never read back.  The records
 * written out are the sanitised ones with the refusal bits.
 *
 * Parameters.
 *   injected mode (io->params_in non-NULL): slot s reads params_in[s]; bit 0 of flags asks for the warp, bits 1 and 2 are ignored.
 *   device mode (params_in NULL): from h(seed, counter, s, j) of the sampler's hash with a FIXED draw number j per field, whether or not
 *   the warp is on; k = h >> 11; a range is lo + k mod (hi - lo + 1):
 *     j = 0 warp on: k * 2^-53 < p_warp;  1 rot in rot_lo..rot_hi;  2 scale;  3 aspect;  4 shear;  5 tx in -tx..tx;  6 ty in -ty..ty;
 *     7 + i the jitter of quad[i] in -jitter..jitter (i = 0..7: jx_0, jy_0, jx_1, ...).  border and fill are the cfg's.
 *   No trigonometry on the device: rot is a row of a host-built bank, device int32 [R][2] = (rint(cos * 65536), rint(sin * 65536)).
 *   The quad, in int64 with arithmetic shifts, for corner k with (px, py) = (-1912,-1912), (1912,-1912), (1912,1912), (-1912,1912)
 *   (119.5 pixels = 1912 / 16):
 *     u = (px * scale * aspect) >> 16;  v = (py * scale) >> 8;  u += (shear * v) >> 8;
 *     x = (cos * u - sin * v + 32768) >> 16;  y = (sin * u + cos * v + 32768) >> 16;
 *     quad[2k] = x + 1912 + tx + jx_k;  quad[2k + 1] = y + 1912 + ty + jy_k, each clamped to +-2^20 as the sanitiser would.
 *   A slot whose warp is off gets the identity quad (and does not read the bank); its other drawn fields are written as drawn.
 *   state = device int64 [2] = (seed, counter), the warper's own; the launch's last act is counter += 1.  The plan's and the
 *   augmenter's draws do not depend on it.
 * dbx_patch_warp_cfg (72 bytes): p_warp 0 (double); rot_lo 8, rot_hi 12; scale_lo 16, scale_hi 20; aspect_lo 24, aspect_hi 28; shear_lo
 * 32, shear_hi 36; tx 40, ty 44, jitter 48 (1/16 pixel, magnitudes); margin 52 (pixels; 8 is the reference's landmark rule); border 56;
 * fill 60; R 64 (rows of the bank); reserved 68 (0). */
typedef struct dbx_patch_warp_rec {
    int32_t flags, border, fill, rot;
    int32_t quad[8];
    int32_t scale, aspect, shear, reserved;
} dbx_patch_warp_rec;
typedef struct dbx_patch_warp_cfg {
    double p_warp;
    int32_t rot_lo, rot_hi, scale_lo, scale_hi, aspect_lo, aspect_hi, shear_lo, shear_hi;
    int32_t tx, ty, jitter, margin, border, fill, R;
    int32_t reserved;
} dbx_patch_warp_cfg;
/* device pointers of dbx_patch_warp_plan (96 bytes: 12 pointers in this order) */
typedef struct dbx_patch_warp_io {
    const int32_t* labels_in;             /* [n][12] */
    const int32_t* count;                 /* [1] */
    const dbx_patch_warp_rec* params_in;  /* [n], or NULL: device mode */
    int64_t* state;                       /* [2] (seed, counter); needed in device mode only */
    const int32_t* rot;                   /* [R][2] (cos, sin) * 65536; needed in device mode with p_warp > 0 only */
    dbx_patch_warp_rec* params;           /* [n] */
    int32_t* labels;                      /* [n][12] */
    float* bbox;                          /* [n][4] */
    float* vertices;                      /* [n][8] */
    float* label;                         /* [n][1] */
    double* fwd;                          /* [n][9] */
    double* inv;                          /* [n][9] */
} dbx_patch_warp_io;
/* cfg is a HOST struct, needed in both modes (injected mode reads margin alone).  Rows at or past min(count, n) are not written.
 * Refused with DBX_ERR_ARG before anything is queued: a null io, cfg or pointer (params_in may be NULL: device mode, which needs state,
 * and with p_warp > 0 the bank), n outside 1..4096, and a cfg with: p_warp outside [0, 1]; a range with lo > hi; scale or aspect outside
 * 1..65535; |shear| above 65535; tx, ty or jitter outside 0..2^16; margin outside 0..119; border outside 0..1; R outside 0..65536; |rot|
 * above 2^20; with p_warp > 0 a rot range that leaves the bank (0 <= rot_lo <= rot_hi < R). */
int dbx_patch_warp_plan(const dbx_patch_warp_io* io, const dbx_patch_warp_cfg* cfg, int32_t n, void* stream);
/* patches, out: device uint8 [n][240][240][c] at any byte address; params / inv / count as dbx_patch_warp_plan left them (or any: the
 * records are sanitised, and whatever inv holds no read leaves the slot's patch).  Slot s < min(count, n) is written, every other byte of
 * out is left alone; a slot with bit 0 clear is copied.  Out of place only.  Refused: a null pointer, c outside 1..4, n outside 1..4096,
 * patches and out overlapping. */
int dbx_patch_warp(const uint8_t* patches, const dbx_patch_warp_rec* params, const double* inv, const int32_t* count, int32_t n, int32_t c,
                   uint8_t* out, void* stream);
/* dbx_patch_warp_plan on the host (the same __host__ __device__ functions) for slots 0 .. count - 1, count in 0..4096: params_in NULL
 * derives from (seed, counter) and rot (a HOST bank).  Refusals as for dbx_patch_warp_plan. */
int dbx_patch_warp_params_host(const dbx_patch_warp_cfg* cfg, int64_t seed, int64_t counter, const dbx_patch_warp_rec* params_in,
                               const int32_t* rot, const int32_t* labels_in, int32_t count, dbx_patch_warp_rec* params, int32_t* labels,
                               float* bbox, float* vertices, float* label, double* fwd, double* inv);
/* dbx_patch_warp of ONE patch [240][240][c] on the host with its record and its inv [9].  Refusals as for dbx_patch_warp. */
int dbx_patch_warp_host(const uint8_t* patch, const dbx_patch_warp_rec* rec, const double* inv, int32_t c, uint8_t* out);

/* ---- data-parallel gradient exchange (new capability; the reference is single-GPU) ----
 * One process per GPU.  Rank 0 makes a 128-byte id (dbx_dp_unique_id) and hands it to the other ranks by any host channel;
 * every rank calls dbx_dp_init with its HIP device current; after each backward, dbx_dp_allreduce_sum_f32 sums the flat fp32
 * gradient buffer (or a bucket of it) over the ranks in place on `stream` -- SUM without division, because the reference
 * loss is a sum over the batch (DenseBox.py:2917).  RCCL over xGMI, resolved by dlopen at first use; the Python front end
 * (densebox_amd/dist.py) drives the same collectives through torch.distributed's "nccl" backend instead. */
int dbx_dp_unique_id(void* id128);
int dbx_dp_init(const void* id128, int32_t rank, int32_t world, void** comm);
int dbx_dp_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
int dbx_dp_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* DENSEBOX_HIP_H */
