/*
 * svc.h — C ABI of the MI355X-native SmartVidCrop saliency-to-crop hot path.
 *
 * libsvc_hip.so (retargetvid_amd/csrc) exports exactly these entry points.  Every
 * data pointer is a DEVICE pointer unless its name ends in _host; the caller owns
 * all buffers, the library owns only the weights and scratch workspace inside the
 * handle.  `stream` is a hipStream_t passed as void* (NULL = the default stream);
 * all work is enqueued on it and nothing synchronises unless stated.  Every call
 * returns 0 on success or a negative SVC_E_* code; svc_last_error() then holds a
 * message for the calling thread.  A call with n = 0 frames / maps / boxes is a
 * successful no-op (its buffers may then be NULL).  The library never exits the
 * process and never reads stdin (the reference blocks on input() at smartVidCrop.py:544-545).
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   svc_create / svc_destroy    unisal_handler.init_unisal_for_images()
 *                               3rd_party_libs/unisal/unisal_handler.py:68-71 and
 *                               Trainer.model / init_unisal_weights, unisal/train.py:1449-1456, :1200-1209
 *   svc_resize_frames_u8        cv2.resize(frame,(SAL_W,SAL_H),INTER_LINEAR), smartVidCrop.py:333-335, :633-635
 *   svc_render_crops_u8         the crop loop of sc_renderer(), smartVidCrop.py:1801-1921 (frame[by1:by2, bx1:bx2, :], :1910)
 *   svc_saliency_u8             unisal_handler.predictions_from_memory_nuint8_np(),
 *                               3rd_party_libs/unisal/unisal_handler.py:85-86 ->
 *                               Trainer.generate_predictions_from_image_memory_nuint8_np, unisal/train.py:1255-1279
 *   svc_threshold_u8            sc_threshold(), smartVidCrop.py:1050-1059
 *   svc_cluster_center          the clustering loop + centre loop of smart_vid_crop():
 *                               sc_clustering_filt() smartVidCrop.py:1062-1161 with the cut blend :2359-2373,
 *                               and sc_find_center_of_mass() :1163-1219 / :2402-2414
 *   svc_iou_i32                 bb_intersection_over_union(), smartVidCrop.py:927-944
 *                               (== retargetvid_eval.py:10-27)
 */
#ifndef SVC_H_
#define SVC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVC_OK 0
#define SVC_E_INVALID (-1)     /* bad argument / unsupported size           */
#define SVC_E_HIP (-2)         /* a HIP runtime call failed                 */
#define SVC_E_BLOB (-3)        /* malformed weights blob                    */
#define SVC_E_NOMEM (-4)

typedef struct SvcHandle SvcHandle;

/* The crop parameters (sc_init_crop_params, smartVidCrop.py:132-209) that the
 * device path consumes. */
typedef struct SvcParams {
    uint32_t struct_size;         /* = sizeof(SvcParams) as the CALLER compiled it: a binding built against an older
                                     layout is rejected with SVC_E_INVALID instead of being read past its end */
    int32_t hdbscan_min;          /* CP['hdbscan_min']  (min_cluster_size)             */
    int32_t hdbscan_min_samples;  /* CP['hdbscan_min_samples'], 0 = None               */
    int32_t select_sum;           /* CP['select_sum']: 1 = cluster sum, else cluster max */
    int32_t op_close;             /* CP['op_close']                                    */
    int32_t clust_filt;           /* CP['clust_filt']: 0 skips filtering, centres only */
    int32_t resize_factor;        /* CP['resize_factor'] (integer, 1 = off): cluster on the map shrunk by this
                                     factor (INTER_LINEAR down, then up again) and take the centre of the
                                     INTER_NEAREST-shrunk map, smartVidCrop.py:1078-1084, :1158, :1184 */
    int32_t com_km;               /* CP['com_km']: 1 = centre of mass (single-cluster K-means = centroid of the non-zero
                                     pixels), 0 = position of the first maximum of the final map in raster order
                                     (sc_find_center_of_mass with km=False, smartVidCrop.py:1165-1178) */
} SvcParams;

/* Per-call diagnostics written by svc_cluster_center when `stats` is non-NULL:
 * int32[n][4] = { points after threshold/blend, clusters selected, label kept, reserved } */
#define SVC_STATS_STRIDE 4

const char *svc_last_error(void);

/* ABI revision of the loaded library (bumped whenever a struct layout or a signature changes); a binding
 * checks it once after dlopen.  2 = SvcParams starts with struct_size and carries resize_factor.
 * 3 = SvcParams ends with com_km; SVC_MAP_HELD is honoured by svc_cluster_center (a v2 library ignores the bit), svc_debug_cluster_state
 *     returns 32 header words, svc_debug_round_plan / svc_debug_argsort_u32 / svc_transnet_* exist.
 * 4 = the host stages svc_host_* (SvcTemporalParams) and svc_saliency_thresholded_u8 exist.
 * 5 = svc_saliency_census_u8, svc_transnet_predict_rows and svc_transnet_config_get / _set exist; svc_create rejects an
 *     unknown spelling of SVC_MX / SVC_SHOT_MX with SVC_E_INVALID.
 * 6 = svc_render_crops_u8 (SVC_RENDER_BGR) and the profile class SVC_K_RENDER exist.
 * 7 = svc_debug_transnet_tap (SVC_SHOT_TAP_*) exists; svc_create rejects SVC_SHOT_M16 outside 2..4 with SVC_E_INVALID.
 * 8 = svc_border_profile_u8, svc_saliency_profile_u8 and the profile class SVC_K_BORDER exist.
 * 9 = svc_resize_frames_nv12 and svc_render_crops_nv12 exist (NV12 input).
 * 10 = svc_render_crops_u8_to_nv12 and svc_render_crops_nv12_to_nv12 exist (NV12 output).
 * 11 = svc_debug_run_node (SVC_NODE_*) exists.
 * 12 = SvcFrameLayout, svc_resize_frames_layout and svc_render_crops_layout exist (pitched frames).
 * (12, no bump) svc_render_crops_filter (SVC_FILTER_*) was added without one: no struct and no existing signature changed, and
 *     a binding finds the entry by its symbol (dlsym), not by the revision.  Likewise svc_debug_net_plan (SVC_PLAN_*), and
 *     SvcColour with svc_resize_frames_colour and svc_render_crops_colour (NV12 colour): a new struct and two new entries; and
 *     svc_render_crops_to_layout (pitched output): one new entry that takes the existing SvcFrameLayout, unchanged, for the output; and
 *     svc_render_windows_q8 (sub-pixel windows): one new entry, no struct; and svc_debug_tail_plan (SVC_TAILPLAN_*): one new test door; and
 *     SVC_NODE_MAP / SVC_NODE_MAP_PROFILE: two new node ids of svc_debug_run_node, which an older library refuses as unknown; and
 *     svc_debug_sort_plan (SVC_SORTPLAN_*): one new test door that takes no handle, no struct; and
 *     svc_focus_jumps_u8 and svc_host_focus_hold (focus stability from resident maps): two new entries, no handle, no struct.
 * 13 = svc_debug_scratch_fill exists.
 * (13, no bump) svc_demo_frames_u8 (SVC_MARK_*: the five-panel demo frames): one new entry, no handle, no struct. */
#define SVC_ABI_VERSION 13
int svc_abi_version(void);

/* Test switch, process-wide (one atomic): byte = -1 switches it off (the default), 0 .. 255 on.  While it is on, every entry that
 * runs device work on a handle's scratch fills that scratch with the byte first -- a hipMemsetAsync on the call's own stream, after
 * the workspace has its size and before the first kernel -- and does so before EVERY pass over the workspace, not once per call:
 * every chunk of a svc_saliency_* call (and svc_debug_run_node), every group of windows of svc_transnet_predict / _predict_rows /
 * svc_debug_transnet_tap, every svc_cluster_center call.  Scratch is the network's activations and per-frame maxima, TransNet's two
 * activation buffers, the tail's shrunk maps and the tail's workspace; the last holds indices and counts and is filled with 0x00
 * whatever the byte, so that a stale read changes a result and never an address.  Weights and their copies, every table, the
 * census totals and the host staging ring are state and are never filled (csrc/svc_internal.h has the list).  The doors that read
 * what the last pass left (svc_debug_tap, svc_debug_cluster_state, svc_threshold_census) fill nothing.
 * A kernel that reads what its pass did not write then reads the fill instead of the previous call's value -- which tests that
 * compare two calls on one handle otherwise make the right one.  0xFF reads as NaN in fp32 and bf16; 0x7F as 3.39e38, which
 * survives a clamp and wins a maximum where NaN does not.
 * Off, an entry pays one relaxed atomic load and launches nothing more; bench.py never turns it on.  (Expected from the code, not
 * measured.)  Process-wide so that every handle of a test session obeys it; not for production.  SVC_E_INVALID outside -1 .. 255. */
int svc_debug_scratch_fill(int byte);

/* weights_blob_host: the packed, BN-folded static SALICON slice of a UNISAL
 * checkpoint (retargetvid_amd.weights.pack_blob).  The blob is copied to `device`. */
int svc_create(const void *weights_blob_host, size_t n_bytes, int device, SvcHandle **out);
int svc_destroy(SvcHandle *h);

/* frames[n][h][w][3] u8 RGB -> out[n][sh][sw][3] u8, OpenCV INTER_LINEAR semantics.  Writes all n * sh * sw * 3 bytes of out and
 * no other byte; out needs no alignment. */
int svc_resize_frames_u8(SvcHandle *h, const uint8_t *frames, int n, int height, int width,
                         uint8_t *out, int sh, int sw, void *stream);

/* frames[n][height][width][3] u8 and boxes[n][4] int32 (x1,y1,x2,y2; x2-x1 == bw, y2-y1 == bh for every frame), both on the
 * device -> out[n][oh][ow][3] u8: each frame's window resampled to oh x ow with OpenCV INTER_LINEAR semantics, i.e.
 * cv2.resize(frame[y1:y2, x1:x2], (ow, oh)); oh == bh && ow == bw is an exact copy (sc_renderer's crop, smartVidCrop.py:1910).
 * flags: SVC_RENDER_BGR swaps R and B (smartVidCrop.py:1894).  Source reads are clamped into the frame (x1 to
 * [0, width - bw], y1 to [0, height - bh]; x2 / y2 are not read), so a bad box never reads outside `frames`.
 * SVC_E_INVALID: bw > width, bh > height, a size < 1, an unknown flag, or a resampled window / output row that needs
 * more than 64 KiB of LDS (2 * (3 bw + 32) + 3 ow + 16 bytes).
 * Writes all n * oh * ow * 3 bytes of out and no other byte, wherever out begins: 16-byte stores are used where the address allows
 * them, and the head and tail of an output row that share a 16-byte word with a neighbour are stored bytewise. */
#define SVC_RENDER_BGR 1
int svc_render_crops_u8(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                        int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream);

/* NV12 input: the two entries above on frames[n][height * 3 / 2][width] u8 -- `height` rows of luma Y, then height / 2 rows of
 * interleaved chroma pairs U V, one pair per 2 x 2 pixels; `height` and `width` are the PICTURE's, even and >= 2 (else
 * SVC_E_INVALID).  Pixel (y, x) takes Y[y][x] and the pair (y >> 1, x >> 1) (chroma replicated, not interpolated) and is
 * converted with BT.601 limited range in 20-bit fixed point, int32, arithmetic shifts (OpenCV's COLOR_YUV2RGB_NV12 constants):
 *   yy = max(0, Y - 16) * 1220542, u = U - 128, v = V - 128
 *   R = clamp((yy + (1 << 19) + 1673527 v) >> 20), G = clamp((yy + (1 << 19) - 852492 v - 409993 u) >> 20),
 *   B = clamp((yy + (1 << 19) + 2116026 u) >> 20), clamp to 0..255
 * fused into the resampling / the copy: out is bit for bit what the _u8 entry gives on the converted frames -- same output
 * layout, flags, clamping of the window origins (which may be odd in x and y: the chroma index comes from frame coordinates)
 * and LDS limit.  They count under SVC_K_RESIZE / SVC_K_RENDER.  No counterpart in the reference (OpenCV decodes to RGB before
 * it sees a frame); the output of these two is RGB / BGR (NV12 output: the _to_nv12 entries below).  BT.709 or full-range
 * frames: svc_resize_frames_colour / svc_render_crops_colour below.  The bytes written are those of the _u8 entries: all of out, nothing else. */
int svc_resize_frames_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width,
                           uint8_t *out, int sh, int sw, void *stream);
int svc_render_crops_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                          int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream);

/* NV12 output: svc_render_crops_u8 / svc_render_crops_nv12 with out[n][oh * 3 / 2][ow] u8 -- oh rows of luma Y, then oh / 2 rows
 * of interleaved pairs U V (row oh + j holds U[j][0] V[j][0] U[j][1] V[j][1] ...: the layout the NV12-input entries read).
 * With C the RGB crop [oh][ow][3] that the entry without _to_nv12 writes (same windows, same clamping of the origins, the
 * exact copy or the INTER_LINEAR resampling), the frame is BT.601 limited range of C in 20-bit fixed point, int32, arithmetic
 * shifts, chroma taken from the SUM of each 2 x 2 block:
 *   Y[y][x] = (269484 r + 528482 g + 102760 b + (16 << 20) + (1 << 19)) >> 20                    r, g, b = C[y][x]
 *   U[j][i] = (-155188 sr - 305135 sg + 460324 sb + (128 << 22) + (1 << 21)) >> 22               sr, sg, sb = sums of r, g, b
 *   V[j][i] = ( 460324 sr - 385875 sg -  74448 sb + (128 << 22) + (1 << 21)) >> 22               over C[2j .. 2j+1][2i .. 2i+1]
 * Y lands in 16..235, U and V in 16..240 (black 16 128 128, white 235 128 128, red 82 90 240): nothing is clamped; decoding
 * a flat colour again with the NV12-input formula gives it back within 2 grey levels.  The transform is fused into the copy / the
 * resampling: no RGB crop is written.  NV12 in, NV12 out is the same definition on the converted crop (every result is
 * that of the converted RGB frames); a plane copy of a native-size window at an even origin would give other bytes and is
 * not done.  SVC_E_INVALID: whatever the RGB entries reject; oh or ow odd or below 2 (a native-size render of a window with
 * an odd bw or bh does not exist: pass an even output size); flags != 0 (SVC_RENDER_BGR has no meaning here); a resampled
 * window that needs more than 64 KiB of LDS per pair of output rows: 2 * (3 bw + 32) + 2 * 3 ow + 3 * (ow + 16) bytes, every
 * term rounded up to 16.  They count under SVC_K_RENDER.  No counterpart in the reference.  Another matrix or range for the
 * output (or the NV12 input): svc_render_crops_colour below.  Writes all n * (oh * 3 / 2) * ow bytes of out and no other byte,
 * wherever out begins. */
int svc_render_crops_u8_to_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                                int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream);
int svc_render_crops_nv12_to_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                                  int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream);

/* Frames in a decoder's layout: the six entries above on frames that are not packed -- a row pitch above the row's bytes, an
 * NV12 chroma plane that starts behind a coded height, frames further apart than their bytes (a hardware decoder's 1920 x 1080
 * surface: pitch 2048, chroma_offset 2048 * 1088; libavcodec's linesize).  `height` and `width` stay the PICTURE's.  Pixel
 * (y, x) of frame f lies at
 *   RGB   frames + f * frame_stride + y * pitch + 3 x
 *   NV12  Y at frames + f * frame_stride + y * pitch + x,  its U V pair at ... + chroma_offset + (y >> 1) * chroma_pitch + (x & ~1)
 * and everything behind the fetched pixel -- conversion, INTER_LINEAR, window rules, the (packed) outputs, the LDS limits -- is
 * that of the packed entries: the result is bit for bit theirs on a packed copy of the same pictures.  out_fmt: SVC_FMT_RGB24
 * (flags: SVC_RENDER_BGR) or SVC_FMT_NV12 (flags 0), the outputs of svc_render_crops_u8 and of the _to_nv12 entries.  The six
 * entries above are these launchers with the packed layout (pitch 3 w | w, chroma_offset w * h, chroma_pitch w, frame_stride
 * 3 w h | w h 3 / 2).
 * Rules, checked before any device work (SVC_E_INVALID, the rule in svc_last_error()): struct_size is this header's; pix_fmt is
 * one of SVC_FMT_*; every value is non-negative; pitch >= the row's bytes (3 w | w); RGB: chroma_offset = chroma_pitch = 0;
 * NV12: chroma_pitch >= w and chroma_offset >= pitch * (h - 1) + w (the chroma plane begins behind the last luma row);
 * frame_stride >= extent, the bytes from a frame's start to the end of its last plane row: pitch * (h - 1) + 3 w for RGB,
 * chroma_offset + chroma_pitch * (h / 2 - 1) + w for NV12; (n - 1) * frame_stride + extent <= PTRDIFF_MAX (the range below is
 * addressed in 64 bits).  No alignment is demanded: an odd pitch is legal.
 * What is read: the kernels load only bytes of [frames, frames + (n - 1) * frame_stride + extent) -- nothing below `frames`,
 * nothing behind the last frame's last plane row, so that range is all that has to be mapped.  Padding bytes inside the range
 * may be loaded (the 16-byte loads are aligned down and guarded by the range's end) and never reach a result.
 * The layout only decides which path runs: the 16-byte paths need `frames` (and, for the copy, `out`) 16-aligned, as for the
 * packed entries, and for NV12 an even frame_stride, chroma_offset and chroma_pitch (a U V pair on an odd address is read
 * by the byte paths).  What is written: all of the packed output, as by the packed entries, and nothing else.
 * They count under SVC_K_RESIZE / SVC_K_RENDER.  No counterpart in the reference. */
#define SVC_FMT_RGB24 0
#define SVC_FMT_NV12  1
typedef struct SvcFrameLayout {
    uint32_t struct_size;     /* sizeof(SvcFrameLayout), as SvcParams: a stale binding is refused */
    int32_t  pix_fmt;         /* SVC_FMT_* */
    int64_t  frame_stride;    /* bytes from frame f to frame f + 1 */
    int64_t  pitch;           /* bytes from row y to row y + 1 (RGB rows; NV12 luma rows) */
    int64_t  chroma_offset;   /* NV12: bytes from the frame's start to its first U V row; RGB: 0 */
    int64_t  chroma_pitch;    /* NV12: bytes between U V rows; RGB: 0 */
} SvcFrameLayout;
int svc_resize_frames_layout(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, int n, int height, int width,
                             uint8_t *out, int sh, int sw, void *stream);
int svc_render_crops_layout(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, int n, int height, int width,
                            const int32_t *boxes, int bw, int bh, uint8_t *out, int out_fmt, int oh, int ow,
                            int flags, void *stream);

/* svc_render_crops_layout with a choice of resampling filter.  Arguments and rules are that entry's: the same layout checks,
 * out_fmt and flags rules, window rules (origins clamped exactly as there) and read range (only bytes of [frames, frames +
 * (n - 1) * frame_stride + extent) are loaded).  Packed frames are passed with the packed layout's values.
 * SVC_FILTER_LINEAR forwards to svc_render_crops_layout: its bytes, its errors.  Any other value but the two below:
 * SVC_E_INVALID ("unknown filter %d").
 * SVC_FILTER_LANCZOS: with (x1, y1) the clamped origin of frame f, the RGB crop is bit for bit
 *   C = PIL.Image.fromarray(frame_rgb[y1:y1+bh, x1:x1+bw]).resize((ow, oh), PIL.Image.LANCZOS)            (Pillow 12.2.0)
 * an a = 3 windowed sinc whose support grows with the shrink factor (antialiased going down, sharp going up), as two 8-bit
 * fixed-point passes: the horizontal pass first, then the vertical one, a u8 intermediate clipped to 0..255 between them;
 * coefficients with 22 fractional bits (normalised in float64, rounded half away from zero), int32 accumulation that starts
 * from 1 << 21, arithmetic shift by 22, clip to 0..255.  A pass whose input and output sizes are equal is skipped (it runs on
 * an identity table: the value itself); when both are equal the call is the exact copy of svc_render_crops_layout.  The
 * filter is cut at the WINDOW's edge, not the frame's (crop first, then resize): pixels outside the window never contribute.
 * NV12 input and pitched layouts change only where a source pixel comes from: the result is that of the converted, packed RGB
 * frames.  out_fmt SVC_FMT_RGB24 with SVC_RENDER_BGR gives C[..., ::-1]; SVC_FMT_NV12 gives the forward transform of C stated
 * at the _to_nv12 entries, unchanged.  No floating point and no global-memory intermediate on the device.
 * One workgroup renders a band of B output rows of one frame out of LDS (B a multiple of R = 1 | 2 rows for an RGB | NV12
 * output): B is the largest value <= 32 for which
 *   2 * span + T(B) * tw + D <= 65536 bytes
 *   span = 3 bw + 32 rounded up to 16          one staged window row (two are staged at a time)
 *   tw   = 3 ow rounded up to 16               one row of the horizontally resampled tile
 *   T(B) = the most window rows the vertical filters of one band of B output rows touch, over the bands of the table:
 *          about B * bh / oh + 6 * max(1, bh / oh) (Pillow's bounds, cut at the window's edge)
 *   D    = 3 ow + 16 (RGB output) | 2 * 3 ow + 3 * (ow + 16), every term rounded up to 16 (NV12 output): the linear path's
 * SVC_E_INVALID, with nothing launched: whatever svc_render_crops_layout rejects (its LDS rule aside); B = R that does not fit
 * (the message carries the byte count); a table with a coefficient of magnitude >= 2^23 or a row with 255 * sum |coefficient|
 * + 2^21 >= 2^31 (the sizes in the message; the 24-bit multiplies and Pillow's int32 range: no size is known to break them).
 * The coefficient tables are built on the host once per handle and (in, out) size of an axis.  Counts under SVC_K_RENDER.
 * No counterpart in the reference (it never resamples its crops). */
#define SVC_FILTER_LINEAR  0
#define SVC_FILTER_LANCZOS 1
int svc_render_crops_filter(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, int n, int height, int width,
                            const int32_t *boxes, int bw, int bh, uint8_t *out, int out_fmt, int oh, int ow,
                            int filter, int flags, void *stream);

/* The colour of NV12 frames: which YUV <-> RGB transform an NV12 source is decoded with and an NV12 output is encoded with.
 * Two matrices (BT.601, BT.709) and two ranges (limited: Y 16..235, U V 16..240; full: 0..255, AVCOL_RANGE_JPEG) give four
 * transforms.  svc_resize_frames_colour is svc_resize_frames_layout with the source's colour; svc_render_crops_colour is
 * svc_render_crops_filter with the source's (in_colour) and the output's (out_colour), chosen independently.  Everything else
 * is those entries': layout rules, window rules, filters, flags, LDS limits, read range, the packed outputs.  Every other
 * entry of this header converts with BT.601 limited and gives the bytes it always gave: it is the entry below with NULL
 * colours, under its own name and with its own errors.
 * The arithmetic has one shape for all four: 20-bit fixed point, int32, arithmetic shifts, clamp to 0..255.  Decode, for a
 * pixel's Y and its replicated U V pair:
 *   yy = max(0, Y - Y0) * CY + (1 << 19),  u = U - 128,  v = V - 128
 *   R = clamp((yy + CVR v) >> 20)   G = clamp((yy + CVG v + CUG u) >> 20)   B = clamp((yy + CUB u) >> 20)
 * Encode, for the RGB crop C (r, g, b = C[y][x]; sr, sg, sb = sums over C[2j .. 2j+1][2i .. 2i+1]):
 *   Y = clamp((YR r + YG g + YB b + (Y0 << 20) + (1 << 19)) >> 20)
 *   U = clamp((UR sr + UG sg + UB sb + (128 << 22) + (1 << 21)) >> 22)        V likewise with VR VG VB
 *
 *   variant        Y0  CY       CVR      CVG      CUG      CUB      | YR     YG     YB     | UR      UG      UB     | VR     VG      VB
 *   bt601 limited  16  1220542  1673527  -852492  -409993  2116026  | 269484 528482 102760 | -155188 -305135 460324 | 460324 -385875 -74448
 *   bt601 full      0  1048576  1470104  -748826  -360853  1858077  | 313524 615514 119538 | -176932 -347356 524288 | 524288 -439026 -85262
 *   bt709 limited  16  1220945  1879825  -558796  -223607  2215014  | 191455 644068 65019  | -105533 -355018 460551 | 460551 -418321 -42230
 *   bt709 full      0  1048576  1651297  -490864  -196424  1945738  | 222927 749942 75707  | -120138 -404150 524288 | 524288 -476214 -48074
 *
 * BT.601 limited keeps the constants OpenCV publishes (three-decimal coefficients; the _nv12 and _to_nv12 entries state them).
 * The other three rows come from the exact rational coefficients: Kr, Kb = 0.299, 0.114 (BT.601) | 0.2126, 0.0722 (BT.709),
 * Kg = 1 - Kr - Kb; S = 255 / 219 and C = 255 / 224 for limited range, 1 and 1 for full.  Each of
 *   CY = S   CVR = 2 (1 - Kr) C   CUB = 2 (1 - Kb) C   CVG = -2 Kr (1 - Kr) C / Kg   CUG = -2 Kb (1 - Kb) C / Kg
 *   YR = Kr / S   YB = Kb / S   UR = -Kr / (2 (1 - Kb) C)   UB = 1 / (2 C)   VR = 1 / (2 C)   VB = -Kb / (2 (1 - Kr) C)
 * is multiplied by 2^20 and rounded half away from zero.  YG = round(2^20 / S) - YR - YB, so white gives exactly 235 (limited)
 * or 255 (full); UG = -UB - UR and VG = -VR - VB, so grey gives exactly 128.
 * Every coefficient is below 2^23 (the kernels' 24-bit multiplies are exact) and every intermediate fits int32 (decode at most
 * 5.8e8 in magnitude, encode 5.2e5 .. 1.074e9).  Limited-range encodes land in 16..235 (Y) and 16..240 (U V) and the clamp
 * never fires; full-range ones reach 256 in U for pure blue and in V for pure red, which the clamp makes 255.  Encoding a flat
 * colour and decoding it with the same variant gives it back within 2 grey levels (limited) or 1 (full).
 * Chroma stays replicated on the way in and summed over 2 x 2 on the way out for every variant: no siting, no interpolation.
 * A NULL colour is BT.601 limited.  SVC_E_INVALID before any device work, the rule in svc_last_error(): struct_size is not this
 * header's; matrix or range is not one of the values below; reserved is not 0; in_colour (colour) is given and layout->pix_fmt
 * is SVC_FMT_RGB24; out_colour is given and out_fmt is SVC_FMT_RGB24 (nothing would read it: pass NULL).
 * The constants travel with the kernel arguments (scalar registers): one kernel set serves the four variants.
 * They count under SVC_K_RESIZE / SVC_K_RENDER.  No counterpart in the reference (it is handed RGB). */
#define SVC_MATRIX_BT601  0
#define SVC_MATRIX_BT709  1
#define SVC_RANGE_LIMITED 0
#define SVC_RANGE_FULL    1
typedef struct SvcColour {
    uint32_t struct_size;     /* sizeof(SvcColour), as SvcParams: a stale binding is refused */
    int32_t  matrix;          /* SVC_MATRIX_* */
    int32_t  range;           /* SVC_RANGE_* */
    int32_t  reserved;        /* 0 */
} SvcColour;
int svc_resize_frames_colour(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *colour, int n,
                             int height, int width, uint8_t *out, int sh, int sw, void *stream);
int svc_render_crops_colour(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *in_colour, int n,
                            int height, int width, const int32_t *boxes, int bw, int bh, uint8_t *out, int out_fmt,
                            const SvcColour *out_colour, int oh, int ow, int filter, int flags, void *stream);

/* Render into an encoder's surfaces: svc_render_crops_colour with a layout for the OUTPUT.  out_layout (required) says where the
 * bytes of the n output frames of oh x ow lie, in the same struct and under the same rules as the frames' layout, applied to the
 * oh x ow picture; its pix_fmt is the output format and takes the place of out_fmt.  Byte 0 of output pixel (y, x) of frame f is
 *   RGB   out + f * frame_stride + y * pitch + 3 x
 *   NV12  Y at out + f * frame_stride + y * pitch + x,  the U V pair of block (j, i) at ... + chroma_offset + j * chroma_pitch + 2 i
 * The contract mirrors the input side: the picture bytes are bit for bit those svc_render_crops_colour writes into a packed
 * output, and EVERY OTHER BYTE of the caller's buffer is left untouched.  What is written is the bytes of every picture row of
 * every plane of the n frames (3 ow bytes per RGB row; ow per luma and per chroma row), all inside [out, out + (n - 1) *
 * frame_stride + extent) -- not the row padding, not the gap between the luma and the chroma plane, not the gap between frames,
 * nothing behind the last frame's extent (its trailing gap need not be mapped).
 * Rules for out_layout, checked before any device work (SVC_E_INVALID, svc_last_error() names the side: "out_layout: ..."): it
 * is not NULL; struct_size is this header's; pix_fmt is one of SVC_FMT_*; every value is non-negative; pitch >= 3 ow | ow;
 * RGB: chroma_offset = chroma_pitch = 0; NV12: chroma_pitch >= ow and chroma_offset >= pitch * (oh - 1) + ow; frame_stride >=
 * extent; (n - 1) * frame_stride + extent <= PTRDIFF_MAX.  No alignment is demanded.  Everything else is
 * svc_render_crops_colour's: the frames' layout, window clamping, filters, flags (by the output format), LDS limits, the read
 * range, the colour rules (out_colour is refused for an RGB out_layout).
 * The layout decides which path runs, never whether the call is legal.  The resampling paths store rows through aligned
 * 16-byte words with bytewise heads and tails at any phase.  The copy's 16-byte path to RGB needs bw >= 16 and out, frame_stride
 * and pitch multiples of 16 (every row start aligned; a row's last group stores exactly its bytes); to NV12 it needs bw % 8 == 0,
 * bw >= 16 and out, frame_stride, pitch, chroma_offset and chroma_pitch multiples of 8; both need the 16-aligned frames of the
 * packed entries.  Anything else -- an odd pitch -- takes the byte path.  An out_layout that holds the packed values (pitch 3 ow |
 * ow, chroma_offset ow * oh, chroma_pitch ow, frame_stride the packed frame's bytes) runs the packed kernels.
 * Counts under SVC_K_RENDER.  No counterpart in the reference. */
int svc_render_crops_to_layout(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *in_colour,
                               int n, int height, int width, const int32_t *boxes, int bw, int bh,
                               uint8_t *out, const SvcFrameLayout *out_layout, const SvcColour *out_colour,
                               int oh, int ow, int filter, int flags, void *stream);

/* Sub-pixel windows: svc_render_crops_to_layout with SVC_FILTER_LINEAR, the top-left corner of every frame's bw x bh window given
 * in 1/256 pixel (origins_q8[n][2] int32 on the device: x, y) instead of by a box.  A crop delivered at a fixed size then follows a
 * smooth trajectory without the steps a whole-pixel origin gives it (a 607 x 1080 window delivered at 1080 x 1920 steps by 1.78
 * output pixels).  Integers only, on the host and on the device; nothing is built per call.
 * Origin.  X = clamp(origins_q8[f][0], 0, (width - bw) * 256), xi = X >> 8, xf = X & 255; Y, yi, yf likewise with height and bh.
 * A bad origin (INT32_MIN, INT32_MAX) never reads outside the frame, as a bad box does not.
 * Columns.  T is the INTER_LINEAR table of (bh, bw) -> (oh, ow) the integer entries use (for equal sizes the identity).  For
 * output column ox it gives the left tap sx in window coordinates (clamped to 0 .. bw - 1, the fraction zero where it was clamped),
 * the right tap min(sx + 1, bw - 1) and the 11-bit weights a0 + a1 = 2048, a1 the right tap's.  xf == 0: taps and weights are the
 * table's, unchanged.  xf > 0:
 *   p = sx * 2048 + a1 + 8 * xf        the table's position in 1/2048 pixel, moved right by xf / 256 pixel
 *   sx' = p >> 11,  a1' = p & 2047,  a0' = 2048 - a1'
 * and the taps are frame columns xi + sx' and xi + sx' + 1, both weighted (no column is a plain copy).  sx' <= bw - 1 (from the
 * table's xmax on, sx = bw - 1 and a1 = 0, and 8 * 255 < 2048), and xf > 0 implies xi < width - bw, so the right tap is at most xi +
 * bw <= width - 1: a pixel of the frame.  At the window's clamped edge columns it is the table's CLAMPED position that is
 * shifted: this is the definition.
 * Rows.  The same with yf, bh and height, on the table's rows as the integer entries fetch them: y0 = clamp(sy, 0, bh - 1), y1 =
 * clamp(sy + 1, 0, bh - 1) with the weights b0 + b1 = 2048.  yf == 0: those rows and weights, unchanged.  yf > 0:
 *   q = y0 * 2048 + (y1 > y0 ? b1 : 0) + 8 * yf        (both rows clamped to one: the position is that row, fraction zero)
 *   sy' = q >> 11,  b1' = q & 2047,  b0' = 2048 - b1',  frame rows yi + sy' and yi + sy' + 1 <= yi + bh <= height - 1
 * Value.  Each channel is the integer entries' blend of the four taps t<row><column>,
 *   h0 = t00 a0 + t01 a1,  h1 = t10 a0 + t11 a1,  clamp((((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2, 0, 255)
 * with the shifted weights.  For NV12 frames each tap is the converted pixel, its chroma index taken from frame coordinates.
 * RGB, BGR and NV12 outputs are made from that RGB crop exactly as by svc_render_crops_to_layout.  oh == bh && ow == bw is NOT a
 * copy here: it runs the same arithmetic on the identity table, a pure fractional shift.
 * Consequence: with every origin a multiple of 256 the output is bit for bit that of svc_render_crops_to_layout (SVC_FILTER_LINEAR)
 * with the boxes (xi, yi, xi + bw, yi + bh).
 * Everything else is svc_render_crops_to_layout's, checked before any device work with the rule in svc_last_error(): the frames'
 * layout rules; out_layout (required; one that holds the packed values runs the packed sinks); the colour rules; flags by the
 * output format; the output contract (all picture bytes and no other byte); the read range [frames, frames + (n - 1) *
 * frame_stride + extent) -- the column xi + bw is loaded only where the frame has it, the row yi + bh only where a phase above zero taps it; n == 0 is a
 * successful no-op; origins_q8 == NULL with n > 0 is SVC_E_INVALID.  The LDS rule is the linear path's with one more staged column:
 * 2 * span + D bytes, span = 3 (bw + 1) + 32 rounded up to 16, D as for the linear path; above 64 KiB the call is refused with the
 * byte count.  Counts under SVC_K_RENDER.  No counterpart in the reference (its windows start on whole pixels). */
int svc_render_windows_q8(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *in_colour,
                          int n, int height, int width, const int32_t *origins_q8 /* [n][2]: x, y */, int bw, int bh,
                          uint8_t *out, const SvcFrameLayout *out_layout, const SvcColour *out_colour,
                          int oh, int ow, int flags, void *stream);

/* The five-panel demo frames of sc_renderer (smartVidCrop.py:1924-2126), composed on the device: per frame the picture, the raw
 * saliency map, the filtered map, the overlay of the two and the picture again, side by side, with integer-defined marks drawn on
 * top.  small[n][ph][pw][3] u8 RGB: the frames ALREADY at the process size (svc_resize_frames_* makes them: the compositor knows
 * nothing of pixel formats, layouts or colours); raw and filt [n_maps][ph][pw] u8 each; map_of[n] int32: the map of frame f; out
 * [n][ph][5 * pw][3] u8.  All pointers are DEVICE pointers.
 * Panels.  Pixel (y, x) of panel k of frame f is out[f][y][k * pw + x].  With S = small[f][y][x], m = map_of[f] (an m outside
 * [0, n_maps) reads as an all-zero map), r = raw[m][y][x], g = filt[m][y][x]:
 *   panel 0: S      panel 1: (r, r, r)      panel 2: (g, g, g)      panel 4: S
 *   panel 3, per channel: the mean of S and g with ties to even,  s = S + g;  v = s >> 1;  v += (s & v & 1)
 * -- what cv2.addWeighted(a, 0.5, b, 0.5, 0) gives through its float path (cvRound of an exact half); OpenCV is not available
 * where this library is built and tested, so that equality is UNPINNED here: the rule above is the definition.
 * Marks.  marks[n_marks][SVC_MARK_WORDS] int32; the marks of frame f are rows first[f] .. first[f + 1] (first[n + 1] int32): both
 * bounds are clamped into [0, n_marks], a negative count is 0, and only the first SVC_DEMO_MAX_MARKS rows of the range are looked at
 * (ignored rows among them count).  They apply in list order, after the panels.  Words of a mark:
 *   { kind | panel << 8,  x0,  y0,  x1,  y1,  p,  q,  r | g << 8 | b << 16 }        coordinates in PANEL pixels
 * A mark is confined to its own panel: it covers only pixels 0 <= x < pw, 0 <= y < ph of that panel, so one that reaches over a
 * panel's edge is cut there and never shows in the neighbour.  It covers pixel P = (x, y) when
 *   SVC_MARK_DISC   (x - x0)^2 + (y - y0)^2 <= p^2
 *   SVC_MARK_LINE   P is within p / 2 of the segment P0 P1 (thickness p), in exact integers: d = P1 - P0, L = d.d, e = P - P0,
 *                   u = e.d;  L == 0 || u <= 0: 4 |e|^2 <= p^2;  else u >= L: 4 |P - P1|^2 <= p^2;  else 4 (e x d)^2 <= p^2 L
 *                   (the kernel forms every product in int64 and the last test as (e x d)^2 <= (p^2 L) >> 2 where |e x d| < 2^31,
 *                   false otherwise: p^2 L < 2^50, so the two are the same statement and nothing overflows)
 *   SVC_MARK_RECT   x0 <= x <= x1 && y0 <= y <= y1 and x == x0 || x == x1 || y == y0 || y == y1 (the 1-pixel outline)
 *   SVC_MARK_TEXT   0 <= x - x0 < w, 0 <= y - y0 < h, with w = q & 0xffff, h = q >> 16: a sprite of coverages, a =
 *                   atlas[p + (y - y0) * w + (x - x0)] (the offset formed in int64); a byte outside [0, atlas_bytes) is not
 *                   read and leaves the pixel alone
 * DISC, LINE and RECT replace the pixel with the mark's colour (the reference writes its "fading" alpha into a BGRA channel that
 * COLOR_BGRA2BGR then drops, :2054: its marks are opaque, and so are these); TEXT blends per channel, c the mark's and d the
 * pixel's value:  (c * a + d * (255 - a) + 127) / 255.
 * A mark is IGNORED -- never a fault, never a read outside the arrays -- when its word 0 is negative, its kind is none of the
 * four or its panel is above 4; when one of x0, y0, x1, y1 is beyond +-32767 (all four are checked for every kind); when p is
 * outside 0 .. 255 for DISC or LINE; when q is negative or a sprite side is above 4096 for TEXT.  Colour bits above 24 are not read.
 * The marks are our own rules, not OpenCV's rasterisers (cv2.circle / cv2.line with LINE_AA, cv2.putText's Hershey glyphs): no
 * anti-aliasing, and the glyphs are whatever the caller puts into the atlas.
 * flags: SVC_RENDER_BGR stores every pixel -- panels and marks -- as (b, g, r): the RGB result with the channels reversed.
 * Contract.  Writes all n * ph * 5 pw * 3 bytes of out and no other byte, wherever out begins (16-byte stores where a row's
 * address allows them, the head and tail of every row bytewise); reads only inside the given arrays, which need no alignment and
 * are left unchanged; out must not overlap them.  n == 0 is a successful no-op.  SVC_E_INVALID with a message, before any launch:
 * a negative n, n_maps or n_marks; ph or pw < 1 (or 15 pw, or the number of workgroups, beyond 2^31 - 1); flags with bits other than
 * SVC_RENDER_BGR; with n > 0 a NULL small, map_of, first or out, NULL raw or filt with n_maps > 0, NULL marks with n_marks > 0,
 * NULL atlas with atlas_bytes > 0.  atlas may be NULL with atlas_bytes == 0 and marks NULL with n_marks == 0.
 * No handle (like svc_focus_jumps_u8): no weights, no scratch, nothing kept between calls; one launch on the caller's stream, on
 * the CURRENT device.  Not counted by the profile classes (they belong to a handle). */
#define SVC_MARK_WORDS 8
#define SVC_DEMO_MAX_MARKS 64
#define SVC_DEMO_PANELS 5
#define SVC_MARK_DISC 0
#define SVC_MARK_LINE 1
#define SVC_MARK_RECT 2
#define SVC_MARK_TEXT 3
int svc_demo_frames_u8(const uint8_t *small /* [n][ph][pw][3] RGB, frames already at process size */, int n, int ph, int pw,
                       const uint8_t *raw, const uint8_t *filt /* [n_maps][ph][pw] each */, int n_maps,
                       const int32_t *map_of /* [n] */,
                       const int32_t *marks /* [n_marks][SVC_MARK_WORDS] */, int n_marks, const int32_t *first /* [n + 1] */,
                       const uint8_t *atlas, size_t atlas_bytes,
                       uint8_t *out /* [n][ph][5 * pw][3] */, int flags /* SVC_RENDER_BGR */, void *stream);

/* frames_nhwc[n][h][w][3] u8 RGB (saliency size, e.g. 140x250) -> maps_nhw[n][h][w] u8.
 * Frame-major output; the reference's [h][w][n] view is a transpose done by the
 * caller only when someone asks for VD['smaps'].
 * height, width >= 8.  The frames are meant to be at the saliency size (svc_resize_frames_u8 brings them there): a larger frame is
 * resampled DOWN to the network size by a kernel that keeps a tile's source rows in LDS, and is refused with SVC_E_INVALID, before
 * anything is launched or the handle's plan changes, when that tile needs more than the CU's 160 KB (the message carries the frame
 * size and the byte count; svc_debug_net_plan reports the count as SVC_PLAN_LZ_LDS).  540x960 is the largest 16:9 frame that runs
 * (143 616 B); 720x1280 (226 272 B) and 1080x1920 are refused.  The other svc_saliency_* entries and svc_debug_run_node plan
 * the same way.  Writes all n * height * width bytes of maps_nhw and no other byte of the caller's; maps_nhw needs no alignment. */
int svc_saliency_u8(SvcHandle *h, const uint8_t *frames_nhwc, int n, int height, int width,
                    uint8_t *maps_nhw, void *stream);

/* svc_saliency_u8 followed by svc_threshold_u8(t) in one pass: the last kernel of the network writes the thresholded map
 * (sc_threshold, smartVidCrop.py:1050-1059, applied to the u8 value as the reference applies it to the stored map).
 * Identical bytes; one launch less per chunk.  t in 0..255 (0 = svc_saliency_u8).  Every byte of maps_nhw is written (a pixel below
 * t as 0). */
int svc_saliency_thresholded_u8(SvcHandle *h, const uint8_t *frames_nhwc, int n, int height, int width,
                                uint8_t *maps_nhw, int t, void *stream);

/* svc_saliency_thresholded_u8 (t in 1..255) that also ADDS, per frame, how many pixels of the UN-thresholded map sit at t - 1, t
 * and t + 1 to the caller's DEVICE rows census_n4[n][4] (uint32; column 3 unused; the caller zeroes them): svc_threshold_census
 * per frame, for callers whose passes mix the frames of several videos (retargetvid_amd/scheduler.py reports the regime
 * diagnostic per video from these rows).  census_n4 may be NULL (= svc_saliency_thresholded_u8).  No counterpart in the reference.
 * maps_nhw is written in full; of census_n4 only columns 0..2 of the n rows are added to (column 3 is neither read nor written). */
int svc_saliency_census_u8(SvcHandle *h, const uint8_t *frames_nhwc, int n, int height, int width,
                           uint8_t *maps_nhw, int t, uint32_t *census_n4, void *stream);

/* The device half of sc_border_detection (smartVidCrop.py:842-924).  The reference takes the maximum of a video's RAW
 * (un-thresholded) maps over time, then per row (f_col) and per column (f_row), and counts the leading / trailing entries
 * that do not exceed t_border.  Here every map i of maps_nhw[n][height][width] is max-combined into the caller's DEVICE row
 * profile_n[i][height + width] (uint32): the first `height` entries are the row maxima (max over x), the next `width` the
 * column maxima (max over y).  The caller zeroes the rows and reduces a video's rows with one maximum over i; counting, the
 * 0.45 cap and the scaling to the original frame (:880-913) are four numbers per video and stay on the host
 * (retargetvid_amd.smartVidCrop.sc_border_detection).  Maximum is order-independent: the rows do not depend on the schedule.
 * Only the n * (height + width) entries of profile_n are touched, each by an atomic maximum (an entry the map does not exceed
 * keeps its value); the maps are only read.  Any width: a thread takes several columns. */
int svc_border_profile_u8(SvcHandle *h, const uint8_t *maps_nhw, int n, int height, int width,
                          uint32_t *profile_n, void *stream);

/* svc_saliency_census_u8 that also fills profile_n (as svc_border_profile_u8 would from the UN-thresholded maps) inside the
 * network's last kernel, for callers that never hold the raw maps (retargetvid_amd/scheduler.py: the frames of several
 * videos share a pass and come out thresholded).  maps_nhw and census_n4 are byte for byte those of svc_saliency_census_u8.
 * t in 0..255 (0 = the plain map); census_n4 may be NULL (required NULL with t = 0); profile_n == NULL takes exactly the
 * launches of svc_saliency_census_u8 / svc_saliency_thresholded_u8.  Written: maps_nhw in full, columns 0..2 of census_n4, the
 * n * (height + width) entries of profile_n (max-combined), nothing else. */
int svc_saliency_profile_u8(SvcHandle *h, const uint8_t *frames_nhwc, int n, int height, int width,
                            uint8_t *maps_nhw, int t, uint32_t *census_n4, uint32_t *profile_n, void *stream);

/* maps[i] = maps[i] < t ? 0 : maps[i], in place.  Only bytes of [maps, maps + n_bytes) are written, whatever the alignment of maps
 * and of n_bytes (a 16-byte access is made only on a whole 16-aligned group inside the range, every other byte on its own);
 * n_bytes = 0 touches nothing. */
int svc_threshold_u8(SvcHandle *h, uint8_t *maps, size_t n_bytes, int t, void *stream);

/* Cluster filter + cut blend + centre of every map, in place on thresholded maps.
 * blend_flags_host[n] (HOST memory, may be NULL), bits per map i:
 *   SVC_BLEND_NEXT  "once map i is final, blend it into map i+1" (smartVidCrop.py:2369-2373; the caller evaluates the
 *                   cut test); map i+1 is then processed after map i;
 *   SVC_MAP_HELD    map i is NOT processed by this call: it is already final (the end of a chain a previous call
 *                   processed, carried over so that the chain can continue: HELD | BLEND_NEXT) or left for a later call.
 *                   A chain that straddles two calls gives the same maps and centres as in one call
 *                   (tests/test_gpu_parity.py::test_blend_chain_carried_over_between_calls).
 * xy[n][2] receives (x, y) centres as float64 in saliency-map pixels, NaN = None (empty map); the entries of held
 * maps are unspecified.  stats may be NULL.
 * What is written: the height * width bytes of every processed map (in place; with resize_factor > 1 the grown map is written
 * back over it) and not one byte of a held map; the xy rows of the processed maps (the row of a held map is left alone or
 * receives a centre of the map as it stands, depending on the settings: do not read it); the stats rows of the processed maps
 * (the row of a held map is left alone).  Nothing outside maps_nhw[n][height][width], xy[n][2] and stats[n][4]. */
#define SVC_BLEND_NEXT 1
#define SVC_MAP_HELD 2
int svc_cluster_center(SvcHandle *h, uint8_t *maps_nhw, int n, int height, int width,
                       const uint8_t *blend_flags_host, const SvcParams *params,
                       double *xy, int32_t *stats, void *stream);

/* Test door, host only (no GPU): the rounds svc_cluster_center plans for a flag array.  round_out[i] = round in which
 * map i is processed, -1 = held; blend0_out[i] = 1 when map i first takes a blend from a held predecessor.
 * Returns the number of rounds (0 when every map is held) or a negative error. */
int svc_debug_round_plan(const uint8_t *flags_host, int n, int32_t *round_out, int32_t *blend0_out);

/* a[n][4], b[n][4] int32 boxes (x1,y1,x2,y2) -> out[n] float64 IoU, inclusive +1 pixel convention.  Writes out[0 .. n) and nothing else. */
int svc_iou_i32(const int32_t *a, const int32_t *b, size_t n, double *out, void *stream);

/* The jump statistics of the focus stability (get_points_on_line and the sums of sc_check_for_extra_cuts, smartVidCrop.py:1337-1455)
 * from maps that stay on the device.  maps_nhw[n][height][width] u8: the FILTERED maps of the n selected frames; xy[n][2] float64
 * (x, y): their centres BEFORE the hold, none of them empty.  sum_cnt[n][2] int32, 8-byte aligned (else SVC_E_INVALID): row i >= 1 =
 * { sum of map i's values at the in-image samples of the move xy[i-1] -> xy[i], number of such samples }; a count of 0 says "no
 * statistic" (the move is below min_d, NumPy would raise on the sample count, or no sample falls inside the image) and comes with
 * sum 0; row 0 = { 0, 0 }.  The caller forms jumps[i] = cnt ? (double)sum / cnt : 255 -- the mean svc_host_focus_stability forms
 * from a float64 accumulator that holds the same integer, so the two agree to the bit (one line walk for both: csrc/svc_jump.h) --
 * and hands the list to svc_host_focus_hold.
 * Domain: both centres of a move finite and no coordinate beyond SVC_FOCUS_MAX_COORD in magnitude; otherwise the row is { 0, -1 }
 * and nothing of the map is read.  That bounds a line at 131 072 samples, so no input makes the kernel run long, and keeps every
 * integer conversion of the walk defined.
 * No handle (like svc_iou_i32): no weights, no scratch, nothing kept between calls; safe to call concurrently from several threads.
 * One launch, one wavefront per map, on the CURRENT device.  Written: all 2 n words of sum_cnt and nothing else.  Read: xy, and of
 * the maps only bytes of [maps_nhw, maps_nhw + n * height * width); the maps need no alignment.  n == 0: a successful no-op.
 * SVC_E_INVALID: n < 0, height or width < 1, min_d NaN, a NULL pointer with n > 0. */
#define SVC_FOCUS_MAX_COORD 65536
int svc_focus_jumps_u8(const uint8_t *maps_nhw, int n, int height, int width, const double *xy, double min_d,
                       int32_t *sum_cnt, void *stream);

/* ---- host stages between the per-frame centres and the crop windows (csrc/svc_host.cpp) ----
 * north_star keeps them on the host; they are native so that a multi-video job runs them off the interpreter lock.
 * No GPU, no handle, no stream: every pointer is HOST memory, float64 unless stated.  Reference: smartVidCrop.py
 *   svc_host_fill_empty_centres  sc_handle_empty_centers :1221-1300.  NaN = no centre; filled in place; returns the
 *                                number of centres still empty (> 0 only when a run copies from an empty neighbour)
 *   svc_host_interp_segment      interp_handler :1528-1548 for the two series of one shot: n samples at the increasing times
 *                                sampled_t -> n_out values at times 0 .. n_out-1 (constant for n < 3, interp1d 'linear' for
 *                                n <= 6, 'quadratic' beyond, both extrapolating)
 *   svc_host_lowpass             sc_butter_lowpass_filter :1599-1627: scipy.signal.filtfilt(b, a, x) with b, a =
 *                                scipy.signal.butter(order, cutoff / (fr / 2)) and zi = scipy.signal.lfilter_zi(b, a)
 *                                (taps = order + 1 coefficients; zi has taps - 1), or, for n <= 3 * taps, the reference's
 *                                5-point moving average over x[2 : n-2]
 *   svc_host_loess               pyloess.Loess(arange(n), y).estimate(j, window, degree) for every j
 *                                (3rd_party_libs/loess/pyloess.py:13-95); NaN where the reference divides 0 / 0
 *   svc_host_savgol              scipy.signal.savgol_filter(y, window, degree), mode 'interp' (:1643)
 *   svc_host_temporal            sc_interpolate + sc_smoothing (:1550-1597, :1648-1734) of one video: centres of the n_sel
 *                                selected frames (true_inds = their frame numbers) + the shots seg[n_seg][2] (first, last
 *                                decoded frame) / seg_sel[n_seg][2] (first, last selected frame) -> interpolated (xi, yi)
 *                                and smoothed (xs, ys) centres, fc values each.  Returns the number of values produced.
 *   svc_host_boxes               sc_compute_bb :979-1048: smoothed centres (saliency-map pixels) -> boxes[fc][4] int64
 *                                (x1, y1, x2, y2), centres[fc][2] (may be NULL) = the truncated full-resolution centres the
 *                                reference writes back to dxs / dys, fbb_wh[2] (may be NULL) = box width, height;
 *                                borders_tblr (may be NULL = 0) = border_t, border_b, border_l, border_r
 *   svc_host_focus_stability     the jump statistics and the focus hold of the ISM 2021 parameter set (get_points_on_line /
 *                                sc_check_for_extra_cuts :1337-1455, the hold loop :2425-2473): centres of the n selected frames (in
 *                                place), the FILTERED maps frame-major uint8 [n][h][w] (host) -> jumps[n] (mean map value along the
 *                                move from centre i-1 to centre i, 255 = none), inds[] = frames with a jump below stab_t (returned
 *                                count); float32 buffer / slope arithmetic as in the reference
 *   svc_host_focus_hold          its second half alone (:2448-2473), for jump statistics that come from svc_focus_jumps_u8: inds[] =
 *                                frames i >= 1 with jumps[i] < stab_t (returned count; room for n), then the hold on the centres, in
 *                                place.  svc_host_focus_stability is its jump loop followed by this call */
typedef struct SvcTemporalParams {
    uint32_t struct_size;       /* = sizeof(SvcTemporalParams) as the caller compiled it */
    int32_t lp_filt;            /* CP['lp_filt'] */
    int32_t lp_taps;            /* CP['lp_order'] + 1 = length of lp_b / lp_a */
    int32_t loess_filt;         /* CP['loess_filt']: 1 = LOESS, 0 = Savitzky-Golay */
    int32_t loess_degree;       /* CP['loess_degree'] */
    int32_t reserved;
    double loess_w_secs;        /* CP['loess_w_secs'] */
    double fr;                  /* frames per second of the video */
} SvcTemporalParams;
int svc_host_focus_stability(double *cx, double *cy, int n, const uint8_t *maps_nhw, int h, int w, double fr, int skip,
                             double min_d_jump, double stab_t, double stab_s, double *jumps, int32_t *inds);
int svc_host_focus_hold(double *cx, double *cy, int n, const double *jumps, double fr, int skip, double stab_t, double stab_s,
                        int32_t *inds);
int svc_host_fill_empty_centres(double *cx, double *cy, int n_sel, const int32_t *seg_sel, int n_seg);
int svc_host_interp_segment(const double *sampled_t, const double *d1, const double *d2, int n, int n_out, double *out1, double *out2);
int svc_host_lowpass(const double *b, const double *a, const double *zi, int taps, const double *x, int n, double *out);
int svc_host_loess(const double *y, int n, int window, int degree, double *out);
int svc_host_savgol(const double *y, int n, int window, int degree, double *out);
int svc_host_temporal(const SvcTemporalParams *p, const double *lp_b, const double *lp_a, const double *lp_zi,
                      const double *cx, const double *cy, int n_sel, const int32_t *true_inds,
                      const int32_t *seg, const int32_t *seg_sel, int n_seg, int fc,
                      double *xi, double *yi, double *xs, double *ys);
int svc_host_boxes(const double *xs, const double *ys, int fc, int w_orig, int h_orig, int w_process, int h_process,
                   int w_final, int h_final, const int32_t *borders_tblr, int64_t *boxes, int64_t *centres, int32_t *fbb_wh);

/* Measurement door (bench.py): record HIP events around every launch of one kernel class on
 * the stream it is launched on.  kernel_class = one of SVC_K_*, or -1 to switch recording off.
 * svc_profile_read synchronises the device, returns the summed duration (ms; 3/4 of the cost of an empty event pair on
 * the same stream, measured at read time, is taken off every launch: calibrated against rocprofv3 kernel durations) and the number of launches recorded since the last
 * read, and resets the log.  Nothing like it exists in the
 * reference (its timers are host wall-clock accumulators, smartVidCrop.py:98-127). */
#define SVC_K_RESIZE 0     /* svc_resize_frames_u8 / _nv12 / _layout / _colour */
#define SVC_K_LANCZOS 1
#define SVC_K_STEM 2
#define SVC_K_PW 3
#define SVC_K_DW 4
#define SVC_K_RESAMPLE 5   /* subsample / upsample / gauss fill / adapt */
#define SVC_K_SMOOTH 6     /* k_smooth_down + k_quantise */
#define SVC_K_THRESHOLD 7
#define SVC_K_COMPACT 8
#define SVC_K_CORE 9
#define SVC_K_PRIM 10
#define SVC_K_FINISH 11
#define SVC_K_RENDER 12    /* svc_render_crops_u8 / _nv12 / _u8_to_nv12 / _nv12_to_nv12 / _layout / _filter / _colour / _to_layout, svc_render_windows_q8 */
#define SVC_K_BORDER 13    /* svc_border_profile_u8 (the fused form, svc_saliency_profile_u8, counts under SVC_K_SMOOTH) */
#define SVC_K_COUNT 14
int svc_profile_enable(SvcHandle *h, int kernel_class);
int svc_profile_read(SvcHandle *h, double *total_ms, int *launches);
/* The same log without the correction: raw_total_ms = sum of the event-pair durations, pair_ms = cost of an empty event pair
 * (median of 15, measured on a stream the handle owns); svc_profile_read returns raw - 0.75 * pair * launches. */
int svc_profile_read_raw(SvcHandle *h, double *raw_total_ms, double *pair_ms, int *launches);

/* Test/diagnostic door: copy internal per-frame clustering state of the LAST
 * svc_cluster_center call to HOST buffers (any may be NULL).  Synchronises.
 *   pts_host[cap]   packed points: row | col<<8 | value<<16, raster order
 *   core_host[cap]  core distances (squared)
 *   mst_host[cap][3] MST edges in Prim order: from, to, weight
 *   labels_host[cap] final labels (-1 = noise)
 *   hdr_host[32]    frame header: the SVC_HDR_* words below
 * Returns the number of points of that frame (or a negative error). */
int svc_debug_cluster_state(SvcHandle *h, int frame, int cap, uint32_t *pts_host, uint32_t *core_host,
                            uint32_t *mst_host, int32_t *labels_host, int32_t *hdr_host);
/* The words of a frame header (int32 each; retargetvid_amd/ops.py carries the same numbers as HDR_*).  Times are in units
 * of 10 ns, measured from the start of the stage that writes them; a range is named by its first word and a count. */
#define SVC_HDR_WORDS        32
#define SVC_HDR_N            0    /* points of the map */
#define SVC_HDR_NSEL         1    /* clusters selected */
#define SVC_HDR_KEPT         2    /* the cluster kept (-1: none) */
#define SVC_HDR_CLUSTERED    3    /* 1: the map went through the cluster filter (clust_filt and more than hdbscan_min + 1 points) */
#define SVC_HDR_NCLUSTERS    4    /* condensed clusters */
#define SVC_HDR_CORE_STAMP0  5    /* k_core: end of phase 1 (thread per point), of phase 2 (wavefront per point), of the kernel */
#define SVC_HDR_CORE_STAMPS  3
#define SVC_HDR_T_SORTED     8    /* k_sort: done */
#define SVC_HDR_T_HIERARCHY  9    /* k_tree / k_tree_par: stabilities summed, clusters selected */
#define SVC_HDR_T_CHOSEN     10   /* ... labels written, kept cluster chosen */
#define SVC_HDR_T_FINISHED   11   /* k_finish: done */
#define SVC_HDR_T_PRIM       12   /* duration of the Prim kernel that took the map */
#define SVC_HDR_T_BUILT      13   /* k_tree: union-find pass done; k_tree_par: row lists of the clusters written */
#define SVC_HDR_TREE_CLOCKS  14   /* k_tree: shader clocks ... */
#define SVC_HDR_T_TREE       15   /* ... during this long (k_tree_par: a copy of T_CHOSEN) */
#define SVC_HDR_LVL_ROUNDS   16   /* k_prim_lvl / k_prim_lvl_big: rounds (0: the map took neither) */
#define SVC_HDR_LVL_RISES    17   /* ... level rises */
#define SVC_HDR_LVL_PHASE0   18   /* k_prim_lvl, SVC_PRIM_LVL=3: time summed per phase (rise, extract, probe, accept + commit, mark) */
#define SVC_HDR_LVL_PHASES   5
#define SVC_HDR_TREE_PAR     23   /* 1: k_tree_par has done the map's hierarchy (0: left to k_tree) */
#define SVC_HDR_T_LVL_SETUP  24   /* k_prim_lvl / k_prim_lvl_big: set-up done */
#define SVC_HDR_TP_STAMP0    25   /* k_tree_par: -, nearest greater ranks, clusters numbered, chains jumped, chain tops (the first is not written) */
#define SVC_HDR_TP_STAMPS    5
#define SVC_HDR_BACK_DONE    30   /* 1: k_tail_back has finished the map (zeroing, CLOSE, centre); k_finish then leaves it alone */

/* Test/diagnostic door: the edge-order routine of the cluster filter (numpy's default argsort, an unstable
 * introsort, emulated on the device; hdbscan sorts the MST edges with it, call site smartVidCrop.py:1099) on
 * arbitrary keys: order_host[p] = index of the key that the sort puts at position p.  n <= 65535.  Synchronises.
 * Returns n (or a negative error). */
int svc_debug_argsort_u32(SvcHandle *h, const uint32_t *keys_host, int n, int32_t *order_host);
/* Test/diagnostic door: what that routine (k_sort and the door above alike) decides from the number of keys alone -- host
 * arithmetic, the very function the kernels carve their working arrays by; needs no handle and no GPU:
 * out[0 .. SVC_SORTPLAN_WORDS) = the SVC_SORTPLAN_* words below.  Returns SVC_SORTPLAN_WORDS.  SVC_E_INVALID: out NULL, cap below
 * SVC_SORTPLAN_WORDS, n outside 1 .. 65535. */
#define SVC_SORTPLAN_IN_LDS 0     /* 1: the 16 bytes per key of working arrays are in LDS (0: in global scratch)           */
#define SVC_SORTPLAN_NSEG 1       /* capacity of the per-range tables: ranges alive at one depth of the recursion          */
#define SVC_SORTPLAN_DEPTH 2      /* the depth limit, 2 * floor(log2 n): a range popped below it is heap-sorted            */
#define SVC_SORTPLAN_LDS_BYTES 3  /* LDS bytes the routine uses: the range tables, and the working arrays when IN_LDS      */
#define SVC_SORTPLAN_WORDS 4
int svc_debug_sort_plan(int n, int32_t *out, int cap);

/* ---- TransNet V1 shot-boundary network ----
 * Replaces ShotTransNet._restore / predict_raw (3rd_party_libs/transnetv1/transnetv1_handler.py:86-97; the reference
 * calls it through predict_frames at smartVidCrop.py:369).
 * svc_transnet_load: the F16 L3 S2 D256 weights as ONE float32 array in the layout of
 *   retargetvid_amd/weights.pack_transnet_blob (per DDCNN cell four [rows][27 taps x channels] GEMM matrices + biases,
 *   Dense(256) and Dense(2) transposed); n_floats is checked.
 * svc_transnet_predict: frames = DEVICE uint8 [n_windows][frames_per_window][27][48][3] (RGB, already 48x27),
 *   probs = DEVICE float32 [n_windows][frames_per_window] = P(transition) of every frame (softmax class 1).
 *   All n_windows * frames_per_window floats of probs are written, and nothing else of the caller's.
 *   Windowing of a video (100-frame windows, stride 50, edge padding) is host logic: transnetv1_handler.predict_video. */
int svc_transnet_load(SvcHandle *h, const float *blob_host, size_t n_floats);
int svc_transnet_predict(SvcHandle *h, const uint8_t *frames, int n_windows, int frames_per_window, float *probs, void *stream);
/* svc_transnet_predict_rows: the same, but the caller keeps only rows row0 .. row1 - 1 of every window (the reference's
 * predict_video keeps rows 25 .. 74 of its 100-frame windows, transnetv1_handler.py:117-121).  Those rows of probs are bit for bit
 * svc_transnet_predict's; the others are UNSPECIFIED (left as they were on the split-bf16 pipes, computed on the fp32 pipe).
 * A cell's temporal reach is 8 frames (its largest dilation), so on the split-bf16 pipes every layer is computed only on the frames
 * the kept rows depend on: 50 / 66 / 82 / 98 of 100 frames in the last four cells = a fifth of the network's FLOPs less.
 * 0 <= row0 < row1 <= frames_per_window.  No store lands outside probs[n_windows][frames_per_window]. */
int svc_transnet_predict_rows(SvcHandle *h, const uint8_t *frames, int n_windows, int frames_per_window, int row0, int row1,
                              float *probs, void *stream);
/* The handle's TransNet knobs as three int32: {matrix pipe: -1 = the handle's SVC_MX | 0 fp32 | 6 bf16x6 | 3 bf16x3, 16-position
 * tiles per wavefront of the split-bf16 cell kernel (2..4), XCD-aware tile order (0 | 1)} -- read from SVC_SHOT_MX / SVC_SHOT_M16 /
 * SVC_SHOT_XCD when the handle is created; ShotTransNet.clone() copies them to the engine of the copy with these two calls instead of
 * going through the process environment.  _set rejects values that are not a configuration with SVC_E_INVALID. */
int svc_transnet_config_get(const SvcHandle *h, int32_t *cfg3);
int svc_transnet_config_set(SvcHandle *h, const int32_t *cfg3);
/* Test/diagnostic door: run svc_transnet_predict_rows on DEVICE frames [n_windows][frames_per_window][27][48][3], stop after
 * `layer` (one of SVC_SHOT_TAP_*), synchronise, and write that layer to the HOST buffer out_host as fp32 NDHWC
 * [n_windows][frames_per_window][H][W][C] without channel padding (split-bf16 planes added as the kernels add them; Dense(256)'s K
 * parts summed in the head's order, then its bias and ReLU).  Frames a layer does not compute (rows outside what row0 .. row1 - 1
 * depend on) are unspecified.  Runs on the null stream.  SVC_E_INVALID: an unknown layer, no weights, more windows than one pass
 * holds, cap_floats below the layer's size. */
#define SVC_SHOT_TAP_INPUT 0   /* [27][48][3]   v / 255                                            */
#define SVC_SHOT_TAP_CELL1 1   /* cells 1..6 (after the ReLU) = 1..6: [27][48][64] x 2, [13][24][128] x 2, [6][12][256] x 2 */
#define SVC_SHOT_TAP_POOL1 7   /* pools 1..3 = 7..9: [13][24][64], [6][12][128], [3][6][256]          */
#define SVC_SHOT_TAP_DENSE 10  /* [256]         Dense(256) after bias and ReLU                       */
int svc_debug_transnet_tap(SvcHandle *h, const uint8_t *frames, int n_windows, int frames_per_window, int row0, int row1, int layer,
                           float *out_host, size_t cap_floats);

/* Test/diagnostic door: copy an intermediate activation of the LAST svc_saliency_u8
 * call (NHWC fp32, frame 0..n-1) to a HOST buffer.  `which` is one of the SVC_TAP_*
 * ids.  Returns the number of floats per frame (or a negative error).  Synchronises. */
#define SVC_TAP_INPUT 0     /* [256][416][3]  normalised network input          */
#define SVC_TAP_FEAT4X 1    /* [32][52][64]   cnn.features.7 output (pre-subsample) */
#define SVC_TAP_FEAT2X 2    /* [16][26][160]  cnn.features.14 output            */
#define SVC_TAP_FEAT1X 3    /* [8][13][1296]  cnn.features.18 output + 16 Gaussian maps */
#define SVC_TAP_POSTCNN 4   /* [8][13][256]                                     */
#define SVC_TAP_DEC 5       /* [32][52][64]   post_upsampling_2 output          */
#define SVC_TAP_PRE 6       /* [h][w]         pre-softmax map at saliency size  */
int svc_debug_tap(SvcHandle *h, int which, int frame, float *out_host, size_t cap_floats);
/* Debug/test entry point: runs ONE node of the saliency network on the caller's input, through the stage function the
 * pass itself calls, on the null stream, and copies the node's output buffer to the host.  Plans (height, width, n) like
 * svc_saliency_u8; n is at most one pass (SVC_CHUNK).  Inputs and outputs are fp32 NHWC host arrays of n frames at the
 * node's level of the network size (NH, NW) that (height, width) selects:
 *   2 .. 17 (SVC_NODE_BLOCK)   cnn.features.<node>: in0 = the block's input, out = what the next block reads (blocks 7 and
 *                              14: behind the ::2 sub-sampling; SVC_NODE_F4X / SVC_NODE_F2X return their full-resolution
 *                              output, the skip branches' input)
 *   SVC_NODE_FRONT             LANCZOS + features.0 + features.1: in0 = uint8 [n][height][width][3], out [NH/2][NW/2][16]
 *   SVC_NODE_F18               in0 [NH/32][NW/32][320] -> the whole row [..][1296]: channels 0..1279 written
 *   SVC_NODE_SKIP_2X / _4X     in0 = F2X [NH/16][NW/16][160] / F4X [NH/8][NW/8][64] -> the whole row of 384 / 192 channels:
 *                              the branch's half (from channel 256 / 128) written
 *   SVC_NODE_POST_CNN          in0 = the whole 1296-channel row -> [NH/32][NW/32][256]
 *   SVC_NODE_US2 / _POST_US2   in0 = the low-resolution tensor ([NH/32][NW/32][256] / [NH/16][NW/16][128]), in1 = the skip half
 *                              ([NH/16][NW/16][128] / [NH/8][NW/8][64]) -> [NH/16][NW/16][128] / [NH/8][NW/8][64]
 *   SVC_NODE_ADAPT             in0 [NH/8][NW/8][64] -> logits [NH/8][NW/8]
 *   SVC_NODE_SMOOTH            in0 = logits -> the pre-softmax map [height][width]
 *   SVC_NODE_MAP               in0 = logits -> [2][height][width]: plane 0 the pre-softmax map (the bytes of SVC_NODE_SMOOTH), plane 1
 *                              the uint8 saliency map's values as floats.  What a pass runs behind the adaptation, in one run: the
 *                              per-frame maxima cleared, the smoothing, then the quantising kernel with threshold 0, no census
 *                              rows and no profile rows into a uint8 buffer of the door's own.
 *   SVC_NODE_MAP_PROFILE       the same with scratch profile rows, so that the kernel of svc_saliency_profile_u8 writes the map.
 *                              A uint8 has no spare value for "not written", so the quantising kernel is launched twice on the one
 *                              pre-softmax map, into a buffer filled with 0x00 and into one filled with 0xFF: a byte that differs
 *                              between the two was not written and comes back as the NaN pattern below.  Both buffers end in 256
 *                              guard bytes of their fill; a guard byte that changed makes the call fail with SVC_E_HIP.
 * Before the node runs, its output buffer and the scratch buffers of the pass are filled with a NaN bit pattern (all ones):
 * whatever the node's kernels do not write -- the other half of a row included -- comes back as that.  Returns the floats
 * per frame of the output.  SVC_E_INVALID, with nothing launched: an unknown node, n outside 1..SVC_CHUNK, in0 (or a
 * decoder node's in1) or out_host NULL, height or width below 8 (as svc_saliency_u8), cap_floats below n frames of output.
 * svc_debug_tap has no pass to read after this call.  Where the call changes the geometry the plan is rebuilt for n frames,
 * so the next pass of more frames re-allocates the workspace. */
#define SVC_NODE_FRONT 1
#define SVC_NODE_BLOCK(idx) (idx)        /* idx = 2 .. 17 */
#define SVC_NODE_F18 18
#define SVC_NODE_SKIP_2X 19
#define SVC_NODE_SKIP_4X 20
#define SVC_NODE_POST_CNN 21
#define SVC_NODE_US2 22
#define SVC_NODE_POST_US2 23
#define SVC_NODE_ADAPT 24
#define SVC_NODE_SMOOTH 25
#define SVC_NODE_MAP 26
#define SVC_NODE_MAP_PROFILE 27
#define SVC_NODE_FULL 100                /* + 7 / 14: the full-resolution output of that block */
#define SVC_NODE_F4X (SVC_NODE_FULL + 7)
#define SVC_NODE_F2X (SVC_NODE_FULL + 14)
int svc_debug_run_node(SvcHandle *h, int node, int n, int height, int width, const void *in0_host, const void *in1_host,
                       float *out_host, size_t cap_floats);
/* Test/diagnostic door: what the plan of a height x width saliency map decides from the shape alone -- host arithmetic, no handle
 * and no device: out[0 .. SVC_PLAN_WORDS) = the SVC_PLAN_* words below (an LDS figure is the dynamic request of a launch in bytes; a
 * *_LDS_MAX figure the most the launcher lets that kernel ask for).  The rows per band are those of a handle created without
 * SVC_SD_ROWS.  Returns SVC_PLAN_WORDS.  SVC_E_INVALID: out NULL, height or width below 8, cap below SVC_PLAN_WORDS.  A shape whose
 * SVC_PLAN_LZ_LDS exceeds SVC_PLAN_LZ_LDS_MAX is reported like any other; svc_saliency_u8 refuses it. */
#define SVC_PLAN_NH 0            /* network input size that (height, width) selects                  */
#define SVC_PLAN_NW 1
#define SVC_PLAN_HKS 2           /* taps of a LANCZOS column / row table (1: the axis is not resampled) */
#define SVC_PLAN_VKS 3
#define SVC_PLAN_FR_OK 4         /* 1: the fused front kernel serves the shape (0: the three kernels)  */
#define SVC_PLAN_FR_NR 5         /* source rows / columns one of its tiles needs at most (0 without it) */
#define SVC_PLAN_FR_NC 6
#define SVC_PLAN_FR_TILES_Y 7    /* its tile rows / columns                                           */
#define SVC_PLAN_FR_TILES_X 8
#define SVC_PLAN_LZ_TILE_CAP 9   /* three-kernel LANCZOS: source rows one workgroup stages at most     */
#define SVC_PLAN_LZ_LDS 10
#define SVC_PLAN_SD_ROWS 11      /* smoothing + resize: map rows per workgroup                         */
#define SVC_PLAN_SD_TILE_CAP 12  /* ... and the network-size rows it stages at most                    */
#define SVC_PLAN_SD_LDS 13
#define SVC_PLAN_FR_LDS 14
#define SVC_PLAN_LZ_LDS_MAX 15
#define SVC_PLAN_SD_LDS_MAX 16
#define SVC_PLAN_FR_LDS_MAX 17
#define SVC_PLAN_WORDS 18
int svc_debug_net_plan(int height, int width, int32_t *out, int cap);
/* Test/diagnostic door: what svc_cluster_center plans for maps of height x width with `params` on this handle, and the compile-time
 * thresholds by which its kernels choose a form per map at run time -- host arithmetic, nothing is launched and the handle is not
 * changed: out[0 .. SVC_TAILPLAN_WORDS) = the SVC_TAILPLAN_* words below.  The plan is made for the shape the tail clusters on
 * (SVC_TAILPLAN_H x SVC_TAILPLAN_W: the map shrunk by resize_factor when the cluster filter is on) and for the handle's tail form
 * (environment SVC_PRIM_LVL / SVC_TREE_PAR / SVC_TAIL_MERGE when it was created).  With these words, a map's point list and
 * its condensed-cluster count, the path of every map through k_core and the hierarchy kernels is determined; the frame header
 * (SVC_HDR_*) records which one it took (tests/tail_paths.py predicts it, tests/test_gpu_tail_paths.py compares).
 * Returns SVC_TAILPLAN_WORDS.  SVC_E_INVALID: h, params or out NULL, cap below SVC_TAILPLAN_WORDS, whatever svc_cluster_center
 * refuses of the shape and of params (struct_size, hdbscan_min, resize_factor, a map that shrinks to nothing). */
#define SVC_TAILPLAN_H 0                  /* the shape the tail clusters on                                              */
#define SVC_TAILPLAN_W 1
#define SVC_TAILPLAN_FUSED 2              /* 1: a round is k_tail_front + k_tail_back (0: one launch per stage)             */
#define SVC_TAILPLAN_LVL_BIG 3            /* 1: k_prim_lvl_big is launched (a map may have more than LVL_CAP points)        */
#define SVC_TAILPLAN_TREE_FALLBACK 4      /* 1: k_tree and k_finish are launched behind (a map may be left to them)         */
#define SVC_TAILPLAN_CAP_CL 5             /* condensed clusters k_tree_par's tables hold, maps of up to TP_CAP_BIG points   */
#define SVC_TAILPLAN_CAP_CL_HUGE 6        /* ... maps of more points                                                        */
#define SVC_TAILPLAN_LVL_CAP 7            /* points: k_prim_lvl up to here, k_prim_lvl_big beyond                           */
#define SVC_TAILPLAN_TP_CAP 8             /* points: k_tree_par with everything in LDS up to here                           */
#define SVC_TAILPLAN_TP_CAP_BIG 9         /* ... with the per-edge arrays partly in the workspace up to here, wholly beyond */
#define SVC_TAILPLAN_TREE_LDS_CAP 10      /* points: k_tree tries its LDS form up to here                                   */
#define SVC_TAILPLAN_TREE_LDS_CLUSTERS 11 /* condensed clusters that form holds (more: k_tree retries in global memory)     */
#define SVC_TAILPLAN_N_RING 12            /* neighbour offsets within RING_R (k_core phase 2 scans them)                    */
#define SVC_TAILPLAN_N_RING1 13           /* ... within RING_R1 (phase 1 walks them)                                        */
#define SVC_TAILPLAN_RING_R 14            /* radius of the ring table: a point with its k-th neighbour beyond goes to phase 3 */
#define SVC_TAILPLAN_RING_R1 15           /* radius of phase 1                                                              */
#define SVC_TAILPLAN_CORE_REG_STEP 16     /* phase 3 in registers: one form per this many points (4 forms) ...              */
#define SVC_TAILPLAN_CORE_REG_MAX 17      /* ... for maps of up to this many points                                         */
#define SVC_TAILPLAN_CORE_LDS_MAX 18      /* the largest N for which phase 3 keeps the points in LDS (beyond: global loop)  */
#define SVC_TAILPLAN_WORDS 19
int svc_debug_tail_plan(const SvcHandle *h, int height, int width, const SvcParams *params, int32_t *out, int cap);
/* SVC_TAP_INPUT with the fused front kernel (the default): the input is written to memory only by handles created
 * with SVC_KEEP_INPUT=1 in the environment; otherwise the call fails with SVC_E_INVALID.
 * svc_front_fused: 1 when the last svc_saliency_u8 call ran LANCZOS + features.0 + features.1 as one kernel
 * (k_front), 0 when as three (SVC_FRONT=0, or a source size whose tiles do not fit in LDS).  bench.py uses it to
 * attribute features.1's FLOPs to the right kernel class. */
int svc_front_fused(const SvcHandle *h);
/* svc_matrix_pipe: which matrix pipe the handle's 1x1-convolution GEMMs (the `pw` kernel class) run on: 0 = fp32 MFMA
 * (v_mfma_f32_32x32x2_f32: exact f32 products, rounds 1-4), 6 = split-bf16 operands on v_mfma_f32_32x32x16_bf16 (every f32
 * operand as three bf16 planes = its 24 significant bits, six plane pairs per product, f32 accumulation: csrc/svc_net.hip,
 * "Split-bf16 operands").  Chosen when the handle is created (environment SVC_MX=f32 | bf16x6; default bf16x6: ~10 %
 * faster, every parity gate of the fp32 pipe unchanged, bit-reproducible with several streams sharing the chip -- the one
 * kernel that was not, the smoothing kernel, computes its bilinear stage with scalar instructions since: DESIGN.md 5); bench.py
 * reports it as roofline.matrix_pipe.  No interface of the reference corresponds to it (its arithmetic type is f32 either way). */
int svc_matrix_pipe(const SvcHandle *h);
/* svc_transnet_matrix_pipe: the same for the TransNet cells with >= 64 input channels (svc_transnet_predict): 0 = fp32 MFMA,
 * 6 = split-bf16 operands, six plane pairs (fp32-class results: |dP| against the oracle 6e-7, the fp32 pipe's 6e-7), 3 = three plane
 * pairs (hi.hi + hi.mid + mid.hi: 16 significant bits per product, |dP| 1.4e-5; opt-in).  Environment SVC_SHOT_MX=f32 | bf16x6 |
 * bf16x3 when the handle is created; default = the handle's SVC_MX.  svc_create rejects any other spelling of SVC_MX / SVC_SHOT_MX
 * with SVC_E_INVALID (ABI 5: a typo used to select the fp32 pipe silently). */
int svc_transnet_matrix_pipe(const SvcHandle *h);
/* svc_threshold_census: the regime diagnostic of the threshold (no counterpart in the reference; smartVidCrop.py:1050-1059 only
 * thresholds).  out[0] = maps that went through svc_saliency_thresholded_u8 on this handle since the last reset, out[1..3] = how
 * many pixels of their UN-thresholded u8 maps sat at t - 1, t and t + 1 (t = the threshold passed to the call).  Two correct
 * fp32 implementations of the network differ by one grey level on ~0.3 % of the pixels; how many pixels that moves across
 * the threshold -- and with them points into or out of the clustering -- is this density.  Measured boundary:
 * ~7 pixels per level and map (trained-like checkpoints) or ~45 (the carrier checkpoint): crop windows identical to the
 * oracle's; ~500 (reference-initialised weights): 21 % of the windows differ by more than a pixel.  Synchronises the device.
 * reset != 0 clears the counters. */
int svc_threshold_census(SvcHandle *h, unsigned long long *out /* [4] */, int reset);

#ifdef __cplusplus
}
#endif
#endif /* SVC_H_ */
