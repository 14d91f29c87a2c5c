// svc_internal.h — handle layout and helpers shared by svc_net.hip / svc_frames.hip / svc_tail.hip / svc_shot.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/svc.h"
#include "svc_devbuf.h"      // DevBuf, ResampleTab; declares svc_set_error

// Division of a 31-bit index by a launch-invariant divisor as multiply + shift: FDiv, make_fdiv and the expression fdiv_q live in
// svc_fdiv.h (no HIP dependency; the tests build it on the host).  Exact for every n < 2^31 and every divisor a launch here uses
// (1 <= d <= 2^31: k_quantise divides by h * w, 106 496 at 416x256 and 518 400 at 540x960); wrong for n >= 2^31, where the
// 64-bit product wraps.  The launcher of k_quantise does not assert n * h * w < 2^31: a handle's chunk (SVC_CHUNK) has
// no upper limit, so the assertion could fire on a call that is accepted today (a default chunk of 32 maps of 540x960 is 2^24).
#include "svc_fdiv.h"
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FDiv &f) { return fdiv_q(n, f.m, f.s); }
__device__ __forceinline__ uint32_t fdivmod(uint32_t n, const FDiv &f, uint32_t &rem) {
    const uint32_t q = fdiv(n, f);
    rem = n - q * f.d;
    return q;
}
#endif

// SVC_NO_PK: a kernel compiled WITHOUT packed-f32 instructions (v_pk_mul/add/fma_f32).  Round 5 found one product lost in a
// `v_pk_mul_f32 x2 ; v_pk_add_f32 ... op_sel:[0,1] op_sel_hi:[1,0]` sequence (a packed instruction that routes the halves of an
// operand CROSSWISE) of the smoothing kernel when a bf16-MFMA workgroup shared the CU (svc_net.hip, sd_bilinear); the trigger is not
// fully understood, so no kernel of the library may contain a half-swapping packed f32 instruction: the kernels whose C code the
// compiler packs that way carry this attribute (the whole library without packed f32 is 1 - 3 % slower: measured, round 6), and
// tools/packed_f32_census.py (run by tests/test_kernel_specs.py) fails the build check if one appears.  Device pass only: the
// host compiler does not know the feature.
#if defined(__HIP_DEVICE_COMPILE__)
#define SVC_NO_PK __attribute__((target("no-packed-fp32-ops")))
#else
#define SVC_NO_PK
#endif

#define SVC_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            svc_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SVC_E_HIP;                                                                  \
        }                                                                                      \
    } while (0)

#define SVC_CHECK_LAUNCH()  SVC_HIP(hipGetLastError())

// The test switch svc_debug_scratch_fill (include/svc.h): -1 = off, 0..255 = the byte every pass fills its SCRATCH with before its
// first kernel.  Process-wide (svc_net.hip holds it), so every handle obeys it; off costs the one relaxed load below and adds no launch.
//
// Which DevBuf is scratch -- its contents mean nothing when a pass starts, so it is filled -- and which is state, never filled:
//   scratch  NetPlan::ws        activations of one network pass.  One exception lives inside it: the Gaussian-prior channels of
//                               CAT1 are constants written once per plan (NetPlan::gauss_filled); a filled pass writes them again
//            NetPlan::fmax      per-frame maxima of one pass: k_adapt clears them, k_smooth_down_mfma raises them
//            SvcHandle::shot_ws TransNet's two ping-pong activation buffers of one pass over a group of windows
//            SvcHandle::rs_maps the shrunk maps of one svc_cluster_center call (resize_factor > 1)
//            SvcHandle::tail_ws the round list and the per-map slots of one svc_cluster_center call.  It holds indices and
//                               counts, so it is always filled with 0x00: a stale read changes a result, never an address
//   state    blob, shot_blob (weights), w_copies, shot_w3, stem_wt, smooth_pad (their re-ordered copies), cvtabs, lztabs, rs_tabs,
//            NetPlan::hb/hk/vb/vk/fr_vt/fr_ht (resampling tables), tail_offsets, tail_ring_cnt, tail_delta (ring tables),
//            NetPlan::lut, NetPlan::gauss (constants of a plan), census (totals that accumulate over calls by contract),
//            depth_pinned (host staging ring: calls still in flight read their slot)
// svc_debug_tap, svc_debug_cluster_state and the census / profile reads look at what the last pass left: they fill nothing.
extern std::atomic<int> g_svc_scratch_fill;
// Fills the whole block (not only what this pass lays out in it) on the pass's stream; byte < 0: the byte asked for.
static inline hipError_t scratch_fill(DevBuf &b, hipStream_t s, int byte = -1) {
    const int f = g_svc_scratch_fill.load(std::memory_order_relaxed);
    if (f < 0 || !b.p) return hipSuccess;
    return hipMemsetAsync(b.p, byte < 0 ? f : byte, b.bytes, s);
}
static inline bool scratch_fill_on() { return g_svc_scratch_fill.load(std::memory_order_relaxed) >= 0; }

struct SvcTensor {
    const float *dev;     // device pointer into the blob
    size_t n;             // floats
};

// One folded layer of the static SALICON graph (weights.fold_state_dict): a 1x1 or a 3x3 depthwise convolution with its bias.
struct SvcLayer {
    int cin, cout, stride, relu6;
    SvcTensor w, b;
};

// An inverted-residual block (MobileNetV2.py:26-83): 1x1 expand (absent where t = 1) -> 3x3 depthwise -> 1x1 project.
struct InvRes {
    SvcLayer expand, dw, project;
    bool has_expand;
    int inp, oup, stride;
};

// The network by name, in the blob's tensor order; filled once by svc_create (svc_net.hip: fill_graph), read by forward_chunk.
struct NetGraph {
    SvcLayer stem;
    InvRes block[17];                     // cnn.features.1 .. features.17: block[i] is features.(i + 1)
    SvcLayer f18, skip2x_expand, skip2x_reduce, skip4x_expand, skip4x_reduce;
    SvcTensor gauss;                      // raw parameters of the Gaussian priors (host copy: SvcHandle::gauss_params)
    InvRes post_cnn, us2, post_us2;       // post_cnn, upsampling_2, post_upsampling_2
    SvcLayer adapt, smooth;               // adaptation 64 -> 1; the smoothing kernel's phase table (w only)
};

struct NetPlan;     // svc_net.hip

struct SvcHandle {
    int device = 0;
    DevBuf blob;
    std::vector<SvcTensor> tensors;
    NetGraph net = {};                    // the layers by name (svc_net.hip: fill_graph)
    std::vector<float> gauss_params;      // coarse_gaussians_salicon [16][2][2]
    // network workspace + plan (svc_net.hip)
    std::unique_ptr<NetPlan> plan;
    // ingest resize tables keyed by (in_h, in_w, out_h, out_w)
    std::map<std::tuple<int, int, int, int>, DevBuf> cvtabs;
    // the renderer's LANCZOS tables keyed by the (in, out) size of one axis (svc_frames.hip: lz_tab; never rewritten)
    std::map<std::pair<int, int>, ResampleTab> lztabs;
    // tail workspace (svc_tail.hip)
    DevBuf tail_ws;
    DevBuf tail_offsets;     // ring-walk offset table
    DevBuf tail_ring_cnt;    // u16[RING_R^2 + 1]: number of offsets with d2 <= index
    int tail_n_offsets = 0, tail_n_offsets1 = 0;
    std::vector<uint32_t> tail_offsets_host;
    std::map<int, DevBuf> tail_delta;  // dr * width + dc of every offset, one table per map width (never rewritten:
                                       // a call still in flight on the stream may be reading the one it was given)
    int tail_frames = 0, tail_h = 0, tail_w = 0;
    size_t tail_frame_stride = 0;      // bytes of per-frame tail workspace
    std::vector<int> tail_slot_of;     // last call: map -> workspace slot (-1: held)
    DevBuf rs_maps;                    // resize_factor != 1: the shrunk maps
    std::map<std::tuple<int, int, int>, std::pair<DevBuf, DevBuf>> rs_tabs;   // (h, w, factor) -> INTER_LINEAR tables down / up
    uint8_t *depth_pinned = nullptr;   // pinned staging ring for the per-map round numbers
    unsigned depth_slot = 0;
    hipEvent_t depth_ev[8] = {};       // recorded behind the upload of a slot; waited on before the slot is rewritten
    std::map<std::tuple<const void *, int, int, int, int>, DevBuf> w_copies;   // re-ordered copies of weight matrices, made on first use (svc_net.hip: weight_copy), keyed by (matrix, row stride, K, padded N, WForm)
    int mx = 6;                        // matrix pipe of the 1x1-convolution GEMMs: 6 = split-bf16 operands, six plane pairs on v_mfma_f32_32x32x16_bf16 (round 5, the default: a pass 1.42 -> 1.24 ms alone, 1.01 -> 0.87 ms with four passes sharing the chip, every parity gate unchanged); 0 = fp32 MFMA (v_mfma_f32_32x32x2_f32, rounds 1-4: SVC_MX=f32).  The one kernel found to miscompute beside bf16 workgroups, the smoothing kernel, lost a product in a packed-instruction sequence of its bilinear stage: written with scalar instructions since (sd_bilinear)
    bool sk_lane = true;               // k_pw_sk / k_dwpw / k_pwpw read their fp32 weights from the lane-order copy (svc_net.hip: lane_form): a wave's load is 1 KB contiguous instead of 32 rows x 32 B (SVC_SK_LANE=0: from the [N][K] matrix)
    std::set<const void *> lds_attr_done;   // kernels whose dynamic-LDS limit has been raised on this handle's device
    int chunk = 32;                    // frames per network pass
    DevBuf census;                     // threshold census (svc_threshold_census): [4] u64 totals, then [chunk][4] u32 per-frame counts of the last pass
    unsigned long long census_maps = 0;
    DevBuf stem_wt;                    // stem weights transposed to [32 out][32 taps, 27 used] for the MFMA stem
    DevBuf smooth_pad;                 // the smoothing phase table padded to [64 phases][56 taps, 49 used]: k_smooth_down_mfma's LDS image
    bool front = true;                 // LANCZOS + features.0 + features.1 as one kernel, k_front (SVC_FRONT=0: three kernels)
    bool keep_input = false;           // ... which then also writes the normalised network input for svc_debug_tap(SVC_TAP_INPUT) (SVC_KEEP_INPUT=1)
    int sd_rows = 0;                   // output rows per workgroup of k_smooth_down_mfma at most (0: SD_ROWS; SVC_SD_ROWS=1..SD_ROWS: the reference of a bit-identity test; the plan shrinks the band further where its LDS would not fit)
    int tail_merge = 1;                // a round's kernels as two fused launches, k_tail_front / k_tail_back (SVC_TAIL_MERGE=0: one launch per stage, for per-kernel profiles)
    int tree_par = 1;                  // data-parallel hierarchy k_tree_par for maps of up to 4352 points (SVC_TREE_PAR=0: the serial builder k_tree)
    int prim_lvl = 1;                  // Prim in rounds, k_prim_lvl / k_prim_lvl_big (SVC_PRIM_LVL=0: one node per step, k_prim_ref, the tests' device reference; 3: k_prim_lvl's phase stamps)
    // TransNet V1 (svc_shot.hip)
    DevBuf shot_blob, shot_ws, shot_w3;   // shot_w3: split-bf16 copies of the cells' weights (svc_shot.hip), valid for shot_w3_mx
    int shot_w3_mx = 0;
    int shot_mx = -1;                  // TransNet cells' matrix pipe: -1 = follow mx, 0 = fp32, 6 = bf16x6, 3 = bf16x3 (SVC_SHOT_MX)
    int shot_m16 = 3;                  // 16-position tiles per wavefront of the split-bf16 cell kernel k_shot_conv_x3m (SVC_SHOT_M16: 2, 3, 4; one more where a wave holds one filter tile)
    int shot_xcd = 1;                  // XCD-aware tile order of k_shot_conv_x3m / k_shot_first_x3 (SVC_SHOT_XCD)
    bool shot_loaded = false;
    // per-kernel-class event log (svc_profile_*)
    int prof_class = -1;
    hipStream_t prof_cal_stream = nullptr;      // a stream of the handle's own for the empty-event-pair calibration of svc_profile_read
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    ~SvcHandle();                      // svc_net.hip, where NetPlan is complete
};

// Records an event pair around the launches in its scope when the class is being profiled.
struct ProfScope {
    SvcHandle *h; hipStream_t s; bool on; hipEvent_t a, b;
    ProfScope(SvcHandle *h_, int cls, hipStream_t s_) : h(h_), s(s_), on(h_->prof_class == cls) {
        if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, s); }
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(b, s); h->prof_events.emplace_back(a, b); } }
};

// Raises a kernel's dynamic-LDS limit, once per kernel and handle: the attribute is per device, so the once-flag lives in the
// handle (one handle = one device), not in the process.
static inline int raise_lds_limit(SvcHandle *h, const void *kfn, int bytes) {
    if (h->lds_attr_done.insert(kfn).second) SVC_HIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return SVC_OK;
}
