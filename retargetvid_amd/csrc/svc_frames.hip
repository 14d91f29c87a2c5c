// svc_frames.hip — frame I/O for gfx950: the ingest down-scale and the renderer, from RGB and NV12 frames (packed, or in a
// decoder's layout: Packed / Pitched below), the renderer to packed RGB / BGR and to NV12.  Every kernel is written once: it
// takes its pixels from a source (SrcRgb<Lay>, SrcNv12<Lay>) and the render kernels hand theirs to a sink (DstRgb<BGR, OLay>,
// DstNv12<OLay>: packed, or in an encoder's layout, the same two policies on the output side); the INTER_LINEAR rule is
// svc_cvlinear.h's.  The one set that is several bodies is the copy path's vector kernel, whose decomposition of the output is the
// sink's own (and, to RGB, the output layout's: a packed output is one run of pixels, a pitched one is rows).
//
// Reference semantics restated per kernel (paths relative to the reference tree):
//   k_cv_resize      cv2.resize(INTER_LINEAR)         smartVidCrop.py:333-335, :633-635
//   k_render_*       frame[by1:by2, bx1:bx2, :] (+ cv2.resize INTER_LINEAR, + RGB2BGR)  smartVidCrop.py:1801-1921
//     k_render_copy_to_rgb, k_render_copy_to_nv12    the copy's vector kernels, one per sink
//     k_render_copy_to_rgb_rows                      the first of them for a pitched output (groups per output row)
//     k_render_copy_px<Src, Dst>                     the copy for everything they leave
//     k_render_resize<Src, Dst>                      the resampled crop
//     k_render_resize_q8<Src, Dst>                   the same at a window origin in 1/256 pixel (no counterpart: svc_render_windows_q8)
//     k_render_lanczos<Src, Dst>                     the crop resampled as PIL.Image.resize(LANCZOS) does it (no counterpart: svc_render_crops_filter)
//   SrcNv12          YUV -> RGB conversion fused into both (no counterpart: the reference is handed RGB)
//   DstNv12          the same crops written as NV12, the forward transform fused in (no counterpart: the reference hands RGB to its writer)
//   Nv12Dec, Nv12Enc the colour (matrix x range: SvcColour) of those two, run-time kernel arguments
//   k_demo_frames    the five panels of the demo video and the marks on them     smartVidCrop.py:1924-2126 (at the end of this file;
//                    a consumer of the down-scale's output beside the renderer: no source, no sink, no handle)
//
// The host layer under the render entries is written once as well: an entry fills a RenderCall and makes one call; render_pair
// states the source x sink pairings (2 x 3) once; the launchers -- render_crops, render_windows, render_crops_lanczos -- are
// launcher<Src, Dst>(call, source layout, output layout) and share their checks and device prologue (render_run); the layout
// entries share render_crops_any and name their launcher by a RenderMode.  The down-scale is one kernel behind resize_frames.
#include <algorithm>
#include <type_traits>

#include "svc_cvlinear.h"
#include "svc_internal.h"
#include "svc_lanczos.h"

// --------------------------------------------------------------------------------------
// loads at arbitrary addresses of a 16-aligned buffer ending at `end`, through aligned 16-byte loads
// --------------------------------------------------------------------------------------
// 16 bytes at a 16-aligned address; the word that runs past `end` is read bytewise, bytes at or past `end` as zero (no
// array: every value stays in a register)
__device__ __forceinline__ uint32_t ld4_end(const uint8_t *p, const uint8_t *end) {
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) v |= (p + i < end ? (uint32_t)p[i] : 0u) << (8 * i);
    return v;
}
__device__ __forceinline__ uint4 ld16_end(const uint8_t *p, const uint8_t *end) {
    if (p + 16 <= end) return *(const uint4 *)p;
    return make_uint4(ld4_end(p, end), ld4_end(p + 4, end), ld4_end(p + 8, end), ld4_end(p + 12, end));
}

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

// the 48 bytes at an arbitrary address a -> o[12] (little-endian dwords): four aligned 16-byte loads, then a funnel shift
// by (a & 15) bytes (two dword-select stages and v_alignbyte_b32)
__device__ __forceinline__ void ld48(const uint8_t *a, const uint8_t *end, uint32_t (&o)[12]) {
    const uint8_t *p = (const uint8_t *)((uintptr_t)a & ~(uintptr_t)15);
    const int s = (int)(a - p), q = s >> 2, b = s & 3;
    // (w, u: vector values, not arrays.  hipcc turns a select between two array elements into one load at a selected
    // address, and the array then lives in scratch -- or, promoted, in LDS -- instead of registers)
    u32x16 w, u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 v = ld16_end(p + 16 * i, end);
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < 14; ++j) u[j] = (q & 2) ? w[j + 2] : w[j];
#pragma unroll
    for (int j = 0; j < 13; ++j) u[j] = (q & 1) ? u[j + 1] : u[j];
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i] = __builtin_amdgcn_alignbyte(u[i + 1], u[i], b);
}

// The 24 bytes at an arbitrary address a -> o0, o1, o2 (little-endian qwords): two aligned 16-byte loads, one qword select
// and a 64-bit funnel shift by (a & 7) bytes.  Bytes past the second word (the last (a & 15) - 8 of o2 when a & 15 > 8)
// read as zero: the callers use 16 bytes (luma) or 18 from an even address (chroma).
__device__ __forceinline__ void ld24(const uint8_t *a, const uint8_t *end, uint64_t &o0, uint64_t &o1, uint64_t &o2) {
    const uint8_t *p = (const uint8_t *)((uintptr_t)a & ~(uintptr_t)15);
    const int s = (int)(a - p), sh = 8 * (s & 7);
    const uint4 v0 = ld16_end(p, end), v1 = ld16_end(p + 16, end);
    const uint64_t a0 = v0.x | ((uint64_t)v0.y << 32), a1 = v0.z | ((uint64_t)v0.w << 32);
    const uint64_t a2 = v1.x | ((uint64_t)v1.y << 32), a3 = v1.z | ((uint64_t)v1.w << 32);
    const bool hi = s & 8;
    const uint64_t b0 = hi ? a1 : a0, b1 = hi ? a2 : a1, b2 = hi ? a3 : a2, b3 = hi ? 0ull : a3;
    o0 = sh ? (b0 >> sh) | (b1 << (64 - sh)) : b0;
    o1 = sh ? (b1 >> sh) | (b2 << (64 - sh)) : b1;
    o2 = sh ? (b2 >> sh) | (b3 << (64 - sh)) : b2;
}

// --------------------------------------------------------------------------------------
// Frame layouts: where the bytes of a source frame -- or of an output frame -- lie (SvcFrameLayout, include/svc.h).  A layout is
// a compile-time policy of the pixel source (Lay, kernel argument L) and of the pixel sink (OLay, kernel argument O) and travels
// behind the kernels' other arguments.  Packed is an empty struct whose offsets are the expressions
// in w that these kernels have always used, so the packed instances are the kernels they were; Pitched carries the four
// strides.  T: the integer type the caller's expression is formed in (size_t for byte loads, ptrdiff_t where x may be < 0).
//   frame<Src>   bytes from frame f to frame f + 1
//   rgb          offset of byte 0 of pixel (y, x) of an RGB frame
//   luma, chroma offsets of Y[y][x] and of the U V pair of pixel (y, x) of an NV12 frame
//   rgb_row      offset of row y of RGB frame f from the buffer's start (the RGB sink's row address: Packed keeps the one
//                expression in ow the sink has always formed it with)
// --------------------------------------------------------------------------------------
struct Packed {
    template <class Src> __host__ __device__ __forceinline__ size_t frame(int h, int w) const { return Src::frame_bytes(h, w); }
    template <class T> __device__ __forceinline__ T rgb(int w, int y, int x) const { return ((T)y * w + x) * 3; }
    template <class T> __device__ __forceinline__ T rgb_row(int f, int h, int w, int y) const { return ((T)f * h + y) * w * 3; }
    template <class T> __device__ __forceinline__ T luma(int w, int y, int x) const { return (T)y * w + x; }
    template <class T> __device__ __forceinline__ T chroma(int h, int w, int y, int x) const { return (T)(h + (y >> 1)) * w + (x & ~1); }
};
struct Pitched {
    long long frame_stride, pitch, chroma_offset, chroma_pitch;
    template <class Src> __host__ __device__ __forceinline__ size_t frame(int, int) const { return (size_t)frame_stride; }
    template <class T> __device__ __forceinline__ T rgb(int, int y, int x) const { return (T)y * (T)pitch + x * 3; }
    template <class T> __device__ __forceinline__ T rgb_row(int f, int, int, int y) const { return (T)f * (T)frame_stride + (T)y * (T)pitch; }
    template <class T> __device__ __forceinline__ T luma(int, int y, int x) const { return (T)y * (T)pitch + x; }
    template <class T> __device__ __forceinline__ T chroma(int, int, int y, int x) const {
        return (T)chroma_offset + (T)(y >> 1) * (T)chroma_pitch + (x & ~1);
    }
};

// --------------------------------------------------------------------------------------
// Colours: the constants of an NV12 frame's YUV <-> RGB transform (SvcColour: a matrix and a range; include/svc.h states the
// table and the rule it is derived by).  They reach the kernels by value with the kernel arguments, so every use is a scalar
// register.  NoColour: what an RGB source or sink takes in their place (an empty struct, like Packed).
// --------------------------------------------------------------------------------------
struct NoColour {};
struct Nv12Dec { int yoff, cy, cvr, cvg, cug, cub; };                   // SrcNv12: nv12_rgb; yoff = (1 << 19) - Y0 * CY
struct Nv12Enc { int yoff, yr, yg, yb, ur, ug, ub, vr, vg, vb; };       // DstNv12: rgb_luma, rgb_chroma; yoff = (Y0 << 20) + (1 << 19)
struct Colours { Nv12Dec dec; Nv12Enc enc; };                           // of a call's source and sink (each takes its part: col)

#define YOFF(y0) (((y0) << 20) + (1 << 19))
#define DOFF(y0, cy) ((1 << 19) - (y0) * (cy)), (cy)
static const Nv12Dec COLOUR_DEC[2][2] = {         // [matrix][range]
    {{DOFF(16, 1220542), 1673527, -852492, -409993, 2116026}, {DOFF(0, 1048576), 1470104, -748826, -360853, 1858077}},
    {{DOFF(16, 1220945), 1879825, -558796, -223607, 2215014}, {DOFF(0, 1048576), 1651297, -490864, -196424, 1945738}}};
#undef DOFF
static const Nv12Enc COLOUR_ENC[2][2] = {
    {{YOFF(16), 269484, 528482, 102760, -155188, -305135, 460324, 460324, -385875, -74448},
     {YOFF(0), 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}},
    {{YOFF(16), 191455, 644068, 65019, -105533, -355018, 460551, 460551, -418321, -42230},
     {YOFF(0), 222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074}}};
#undef YOFF
static const Colours COLOURS_DEFAULT = {COLOUR_DEC[SVC_MATRIX_BT601][SVC_RANGE_LIMITED], COLOUR_ENC[SVC_MATRIX_BT601][SVC_RANGE_LIMITED]};

// One SvcColour of a call, checked (`what`: "colour", "in_colour", "out_colour") -> its indices.  NULL: BT.601 limited.  A
// colour given for an RGB side (`nv12` false) is refused: nothing there would read it.  Plain comparisons, before any device work.
static int colour_check(const char *name, const char *what, const SvcColour *c, bool nv12, int &matrix, int &range) {
    matrix = SVC_MATRIX_BT601;
    range = SVC_RANGE_LIMITED;
    if (!c) return SVC_OK;
    if (c->struct_size != sizeof(SvcColour)) {
        svc_set_error("%s: %s: SvcColour.struct_size is %u, this library's is %zu (a stale binding)", name, what, c->struct_size, sizeof(SvcColour));
        return SVC_E_INVALID;
    }
    if (c->matrix != SVC_MATRIX_BT601 && c->matrix != SVC_MATRIX_BT709) {
        svc_set_error("%s: %s: unknown matrix %d (SVC_MATRIX_BT601 or SVC_MATRIX_BT709)", name, what, c->matrix);
        return SVC_E_INVALID;
    }
    if (c->range != SVC_RANGE_LIMITED && c->range != SVC_RANGE_FULL) {
        svc_set_error("%s: %s: unknown range %d (SVC_RANGE_LIMITED or SVC_RANGE_FULL)", name, what, c->range);
        return SVC_E_INVALID;
    }
    if (c->reserved != 0) {
        svc_set_error("%s: %s: reserved is %d, it must be 0", name, what, c->reserved);
        return SVC_E_INVALID;
    }
    if (!nv12) {
        svc_set_error("%s: %s is given but that side is rgb24: a colour describes NV12 frames (pass NULL)", name, what);
        return SVC_E_INVALID;
    }
    matrix = c->matrix;
    range = c->range;
    return SVC_OK;
}

// --------------------------------------------------------------------------------------
// Pixel sources: what the kernels below ask of a frame format, in the layout Lay (`L`: the kernel's layout argument).
//   size_ok, size_rule   the pictures the format can hold, and the words the error text says it with
//   frame_bytes          bytes of one packed frame
//   extent               bytes from a frame's start to the end of its last plane row: the kernels read inside
//                        [frames, frames + (n - 1) * L.frame + extent) and nowhere else
//   vec_ok               whether the 16-byte paths (px16, stage_row's vec) may run on this layout
//   colour, col          the colour constants the source converts with (a kernel argument, K below; NoColour for RGB) and the
//                        source's part of a Colours pair
//   px<BGR>              pixel (y, x) of the frame at `fr` as r | g << 8 | b << 16 (BGR: b | g << 8 | r << 16), byte loads
//   px16<BGR>            pixels x .. x + 15 of row y as 48 bytes (o[12], little-endian dwords) through aligned 16-byte loads
//                        (the buffer is 16-aligned and ends at `end`).  x may be below 0 by less than 16 (the copy kernel's
//                        second run): then the pixels left of the row are whatever lies there and the caller masks them
//                        out.  They lie inside the buffer, also with padding and for row 0: that run is never the first
//                        window row of frame 0, so its row starts at least one pitch (a row further down the same frame) or
//                        one frame stride (row 0 of the next frame) behind `frames`, and it reaches back by k < 16 pixels
//                        with k <= bw <= w, i.e. by at most 3 w <= pitch <= extent <= frame stride bytes (NV12: k <= w <=
//                        pitch for luma; at most 16 <= w <= chroma_offset bytes for chroma, bw >= 16 on that path).  The
//                        16-byte words are aligned down from there and `frames` is 16-aligned, so no load starts below it.
//   order16<BGR>         what is left to do to such 48 bytes once two runs are merged: px16 then order16 is the output's
//                        channel order
//   stage_row            pixels x .. x + bw - 1 of row y as RGB bytes into the LDS row `row` (span_cap bytes) by the whole
//                        workgroup (vec: frames 16-aligned, 16-byte loads; else bytewise); returns the byte of `row` at which
//                        they start
// --------------------------------------------------------------------------------------
template <class Lay>
struct SrcRgb {                                 // u8 [h][w][3]; Pitched: rows `pitch` bytes apart
    typedef Lay lay;
    typedef NoColour colour;
    static colour col(const Colours &) { return NoColour(); }
    static bool size_ok(int h, int w) { return h >= 1 && w >= 1; }
    static const char *size_rule() { return ""; }
    __host__ __device__ static size_t frame_bytes(int h, int w) { return (size_t)h * w * 3; }
    static size_t extent(const Packed &, int h, int w) { return frame_bytes(h, w); }
    static size_t extent(const Pitched &L, int h, int w) { return (size_t)L.pitch * (h - 1) + (size_t)w * 3; }
    static bool vec_ok(const Lay &) { return true; }        // ld48 takes any address

    template <bool BGR>
    __device__ __forceinline__ static uint32_t px(const uint8_t *__restrict__ fr, const Lay &L, const colour &, int h, int w, int y, int x) {
        const uint8_t *s = fr + L.template rgb<size_t>(w, y, x);
        const uint32_t c0 = s[0], c1 = s[1], c2 = s[2];
        return BGR ? c2 | (c1 << 8) | (c0 << 16) : c0 | (c1 << 8) | (c2 << 16);
    }

    // one 48-byte run of the row, as it lies there
    template <bool BGR>
    __device__ __forceinline__ static void px16(const uint8_t *__restrict__ fr, const Lay &L, const colour &, int h, int w, int y, int x,
                                                const uint8_t *end, uint32_t (&o)[12]) {
        ld48(fr + L.template rgb<ptrdiff_t>(w, y, x), end, o);
    }

    // BGR: a fixed byte permutation inside the group (it starts on a pixel boundary)
    template <bool BGR>
    __device__ __forceinline__ static void order16(uint32_t (&o)[12]) {
        if (!BGR) return;
        uint32_t t[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * i + j, c = d % 3, sb = d - c + 2 - c;      // R <-> B inside the pixel
                v |= ((o[sb >> 2] >> (8 * (sb & 3))) & 0xffu) << (8 * j);
            }
            t[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = t[i];
    }

    // vec: the aligned 16-byte words that hold the span, so the row starts at the span's own 16-byte phase
    __device__ __forceinline__ static int stage_row(const uint8_t *__restrict__ fr, const Lay &L, const colour &, int h, int w, int y, int x,
                                                    int bw, uint8_t *row, int span_cap, const uint8_t *end, int vec) {
        const uint8_t *a = fr + L.template rgb<size_t>(w, y, x);
        const int span = bw * 3;
        if (vec) {
            const uint8_t *p = (const uint8_t *)((uintptr_t)a & ~(uintptr_t)15);
            const int sh = (int)(a - p), nw = (sh + span + 15) >> 4;
            for (int i = threadIdx.x; i < nw; i += 256) ((uint4 *)row)[i] = ld16_end(p + 16 * i, end);
            return sh;
        }
        for (int i = threadIdx.x; i < span; i += 256) row[i] = a[i];
        return 0;
    }
};

// NV12 (no counterpart in the reference: its frames are decoded to RGB by OpenCV before it sees them).  A frame of a
// height x width picture is u8 [height * 3 / 2][width]: `height` luma rows, then height / 2 rows of interleaved U V pairs;
// pixel (y, x) takes Y[y][x] and the pair (y >> 1, x >> 1).  The conversion is 20-bit fixed point in the frames' colour
// (Nv12Dec: BT.601 or BT.709, limited or full range; include/svc.h states the table); everything behind it -- the
// INTER_LINEAR arithmetic, the window rules, the output layouts -- is shared with the RGB source, so the results are the RGB
// source's on the converted frames.  Another matrix or range changes the constants and nothing else, so they are a kernel
// argument (wave-uniform: scalar registers), not a template parameter: the kernels are bound by memory, and a compile-time
// colour would multiply the NV12 -> NV12 instances by 16.
#define NV12_SHIFT 20
#define NV12_C0 128

// one pixel -> r | g << 8 | b << 16 (BGR: b | g << 8 | r << 16); int32 throughout (largest magnitude 5.8e8)
template <bool BGR>
__device__ __forceinline__ uint32_t nv12_rgb(const Nv12Dec &K, int Y, int U, int V) {
    // (__mul24: both factors fit 24 bits and the products 32, so the full-rate 24-bit multiply is exact)
    // yy = max(0, Y - Y0) * CY + (1 << 19), taken as max(Y * CY + yoff, 1 << 19): the same number for every Y (CY > 0)
    const int yy = max(__mul24(Y, K.cy) + K.yoff, 1 << (NV12_SHIFT - 1)), u = U - NV12_C0, v = V - NV12_C0;
    // clamp(x >> 20, 0, 255) taken as clamp(x, 0, 2^28 - 1) >> 20 (the same value).  Written the first way, hipcc turns two
    // clamped shifts that are packed next to each other into one v_ashr_pk_u8_i32 and then relies on the upper half of its
    // result being zero, which it is not on gfx950 (seen as stray bits in bytes 2 and 3 of every third output dword).
    const int top = (256 << NV12_SHIFT) - 1;
    const int r = min(max(yy + __mul24(K.cvr, v), 0), top) >> NV12_SHIFT;
    const int g = min(max(yy + __mul24(K.cvg, v) + __mul24(K.cug, u), 0), top) >> NV12_SHIFT;
    const int b = min(max(yy + __mul24(K.cub, u), 0), top) >> NV12_SHIFT;
    return BGR ? (uint32_t)(b | (g << 8) | (r << 16)) : (uint32_t)(r | (g << 8) | (b << 16));
}

template <class Lay>
struct SrcNv12 {                                // u8 [h * 3 / 2][w]; Pitched: luma rows `pitch` apart, U V rows `chroma_pitch` apart from `chroma_offset`
    typedef Lay lay;
    typedef Nv12Dec colour;
    static colour col(const Colours &c) { return c.dec; }
    static bool size_ok(int h, int w) { return h >= 2 && w >= 2 && !(h & 1) && !(w & 1); }       // even, >= 2
    static const char *size_rule() { return " (height and width of an NV12 picture are even)"; }
    __host__ __device__ static size_t frame_bytes(int h, int w) { return (size_t)(h + h / 2) * w; }
    static size_t extent(const Packed &, int h, int w) { return frame_bytes(h, w); }
    static size_t extent(const Pitched &L, int h, int w) { return (size_t)L.chroma_offset + (size_t)L.chroma_pitch * (h / 2 - 1) + (size_t)w; }
    // px16 takes its 18 chroma bytes from an EVEN address (ld24 delivers 17 from an odd one).  `frames` is 16-aligned on that
    // path, so every U V pair lies on an even address iff these three are even; a layout with an odd one takes the byte paths.
    static bool vec_ok(const Packed &) { return true; }
    static bool vec_ok(const Pitched &L) { return !((L.frame_stride | L.chroma_offset | L.chroma_pitch) & 1); }

    template <bool BGR>
    __device__ __forceinline__ static uint32_t px(const uint8_t *__restrict__ fr, const Lay &L, const colour &K, int h, int w, int y, int x) {
        const uint8_t *c = fr + L.template chroma<size_t>(h, w, y, x);
        return nv12_rgb<BGR>(K, fr[L.template luma<size_t>(w, y, x)], c[0], c[1]);
    }

    // the 16 luma bytes and the 18 bytes that hold their (at most nine) chroma pairs, each through two aligned 16-byte
    // loads; the chroma index is taken from frame coordinates, so x and y may be odd
    template <bool BGR>
    __device__ __forceinline__ static void px16(const uint8_t *__restrict__ fr, const Lay &L, const colour &K, int h, int w, int y, int x,
                                                const uint8_t *end, uint32_t (&o)[12]) {
        uint64_t Y[3], C[3];
        ld24(fr + L.template luma<ptrdiff_t>(w, y, x), end, Y[0], Y[1], Y[2]);
        ld24(fr + L.template chroma<ptrdiff_t>(h, w, y, x), end, C[0], C[1], C[2]);      // (x & ~1 = 2 * (x >> 1), also for x < 0)
        const bool odd = x & 1;
        uint32_t p[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            // pair of pixel i = (i + odd) >> 1: i / 2 for even i, (i - 1) / 2 + odd for odd i; pair p = bytes 2 p, 2 p + 1 of C
            const int p0 = i >> 1, p1 = (i + 1) >> 1;
            const uint32_t h0 = (uint32_t)(C[p0 >> 2] >> (16 * (p0 & 3))) & 0xffffu, h1 = (uint32_t)(C[p1 >> 2] >> (16 * (p1 & 3))) & 0xffffu;
            const uint32_t uv = (i & 1) && odd ? h1 : h0;
            p[i] = nv12_rgb<BGR>(K, (int)((Y[i >> 3] >> (8 * (i & 7))) & 0xffu), (int)(uv & 0xffu), (int)(uv >> 8));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                     // four pixels = three dwords
            o[3 * i] = p[4 * i] | (p[4 * i + 1] << 24);
            o[3 * i + 1] = (p[4 * i + 1] >> 8) | (p[4 * i + 2] << 16);
            o[3 * i + 2] = (p[4 * i + 2] >> 16) | (p[4 * i + 3] << 8);
        }
    }

    template <bool BGR>
    __device__ __forceinline__ static void order16(uint32_t (&)[12]) {}      // converted straight to the order asked for

    // the row is converted while it is staged; vec: 16 pixels per thread through px16
    __device__ __forceinline__ static int stage_row(const uint8_t *__restrict__ fr, const Lay &L, const colour &K, int h, int w, int y, int x,
                                                    int bw, uint8_t *row, int span_cap, const uint8_t *end, int vec) {
        if (vec) {
            for (int g = threadIdx.x; 16 * g < bw; g += 256) {
                uint32_t o[12];
                px16<false>(fr, L, K, h, w, y, x + 16 * g, end, o);
#pragma unroll
                for (int j = 0; j < 3; ++j)                     // (the last group's words past the row's capacity are never read)
                    if (48 * g + 16 * j + 16 <= span_cap) ((uint4 *)(row + 48 * g))[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
            }
        } else {
            for (int i = threadIdx.x; i < bw; i += 256) {
                const uint32_t v = px<false>(fr, L, K, h, w, y, x + i);
                row[3 * i] = (uint8_t)v;
                row[3 * i + 1] = (uint8_t)(v >> 8);
                row[3 * i + 2] = (uint8_t)(v >> 16);
            }
        }
        return 0;
    }
};

// --------------------------------------------------------------------------------------
// ingest down-scale: OpenCV INTER_LINEAR on u8, one thread per output pixel, the four tapped source pixels by byte loads
// (at 4K -> 140x250 a frame is tapped at 140 000 of its 8.3 M pixels)
// --------------------------------------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(256) void k_cv_resize(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                   const int *__restrict__ tab, int n, int h, int w, int oh, int ow,
                                                   const typename Src::lay L, const typename Src::colour K) {
    const CvLinear T(tab, oh, ow);
    size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    size_t total = (size_t)n * oh * ow;
    if (gid >= total) return;
    int ox = gid % ow;
    int oy = (gid / ow) % oh;
    int f = gid / ((size_t)ow * oh);
    int y0, y1, b0, b1, sx, sx1, a0, a1;
    bool inner;
    T.row(oy, h, y0, y1, b0, b1);
    T.col(ox, w, sx, sx1, a0, a1, inner);
    const uint8_t *fr = in + f * L.template frame<Src>(h, w);
    const uint32_t p00 = Src::template px<false>(fr, L, K, h, w, y0, sx), p01 = Src::template px<false>(fr, L, K, h, w, y0, sx1);
    const uint32_t p10 = Src::template px<false>(fr, L, K, h, w, y1, sx), p11 = Src::template px<false>(fr, L, K, h, w, y1, sx1);
    uint8_t *o = out + gid * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        o[c] = CvLinear::blend((p00 >> (8 * c)) & 0xffu, (p01 >> (8 * c)) & 0xffu, (p10 >> (8 * c)) & 0xffu, (p11 >> (8 * c)) & 0xffu,
                               a0, a1, b0, b1, inner);
}

// the INTER_LINEAR table of (height, width) -> (sh, sw), built once per handle and size pair (the ingest's and the
// renderer's tables are the same thing: a window of bh x bw is resampled exactly like a frame of that size)
static int cv_tab(SvcHandle *h, int height, int width, int sh, int sw, const int **out) {
    auto key = std::make_tuple(height, width, sh, sw);
    auto it = h->cvtabs.find(key);
    if (it == h->cvtabs.end()) {
        const std::vector<int> tab = cv_linear_tab(height, width, sh, sw, (double)height / sh, (double)width / sw);
        DevBuf buf;
        int rc = buf.ensure(tab.size() * 4);
        if (rc) return rc;
        SVC_HIP(hipMemcpy(buf.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        it = h->cvtabs.emplace(key, std::move(buf)).first;
    }
    *out = (const int *)it->second.p;
    return SVC_OK;
}

template <class Src>
static int resize_frames(const char *name, SvcHandle *h, const uint8_t *frames, const typename Src::lay &L, const Colours &C, int n,
                         int height, int width, uint8_t *out, int sh, int sw, void *stream) {
    if (!h || n < 0 || (n > 0 && (!frames || !out)) || !Src::size_ok(height, width) || sh < 1 || sw < 1) {     // n = 0: a no-op, null buffers allowed
        svc_set_error("%s: invalid argument%s", name, Src::size_rule());
        return SVC_E_INVALID;
    }
    if (n == 0) return SVC_OK;
    SVC_HIP(hipSetDevice(h->device));
    const int *tab = nullptr;
    int rc = cv_tab(h, height, width, sh, sw, &tab);
    if (rc) return rc;
    size_t total = (size_t)n * sh * sw;
    ProfScope ps(h, SVC_K_RESIZE, (hipStream_t)stream);
    k_cv_resize<Src><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(
        frames, out, tab, n, height, width, sh, sw, L, Src::col(C));
    SVC_CHECK_LAUNCH();
    return SVC_OK;
}

extern "C" int svc_resize_frames_u8(SvcHandle *h, const uint8_t *frames, int n, int height, int width,
                                    uint8_t *out, int sh, int sw, void *stream) {
    return resize_frames<SrcRgb<Packed>>("svc_resize_frames_u8", h, frames, Packed(), COLOURS_DEFAULT, n, height, width, out, sh, sw, stream);
}
extern "C" int svc_resize_frames_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width,
                                      uint8_t *out, int sh, int sw, void *stream) {
    return resize_frames<SrcNv12<Packed>>("svc_resize_frames_nv12", h, frames, Packed(), COLOURS_DEFAULT, n, height, width, out, sh, sw, stream);
}

// --------------------------------------------------------------------------------------
// render: every frame's window (x1, y1, bw, bh) of the full frames, copied or resampled to oh x ow
// (sc_renderer, smartVidCrop.py:1801-1921: frame[by1:by2, bx1:bx2, :] at :1910, the BGR conversion of the pickle mode :1894)
// --------------------------------------------------------------------------------------
// The window origin of frame f, clamped so that every source read lies inside that frame (the host checked bw <= width,
// bh <= height); x2 / y2 of the box are not read.
__device__ __forceinline__ void render_origin(const int32_t *__restrict__ boxes, int f, int height, int width, int bh, int bw,
                                              int &x0, int &y0) {
    x0 = min(max(boxes[4 * f], 0), width - bw);
    y0 = min(max(boxes[4 * f + 1], 0), height - bh);
}

// nb bytes of an output row from LDS (orow, at the phase of dst: orow & 15 == dst & 15) to dst by the whole workgroup: aligned
// 16-byte stores; bytes [0, head) and [head + 16 * nw, nb) are partial 16-byte words of the output: bytewise
__device__ __forceinline__ void row_out(uint8_t *__restrict__ dst, const uint8_t *orow, int nb) {
    const int head = min(nb, (16 - (int)((uintptr_t)dst & 15)) & 15), nw = (nb - head) >> 4;
    const uint4 *src4 = (const uint4 *)(orow + head);
    uint4 *dst4 = (uint4 *)(dst + head);
    for (int i = threadIdx.x; i < nw; i += 256) dst4[i] = src4[i];
    for (int i = threadIdx.x; i < head; i += 256) dst[i] = orow[i];
    for (int i = head + 16 * nw + threadIdx.x; i < nb; i += 256) dst[i] = orow[i];
}

// The two vector kernels of the copy path (output size == window size), one per sink; frames and out are 16-aligned.
// To RGB, bw >= 16.  The output is one packed run of pixels;
// thread g owns output pixels [16 g, 16 g + 16) = bytes [48 g, 48 g + 48), written as three aligned 16-byte stores.  The
// group's source is one run of 16 pixels of the window row it starts in (Src::px16), and when the group runs over the end
// of that row, the rest comes from the next window row (of this frame or the next one) through a second run, placed so
// that its pixel k is the first of that row, merged in by byte mask.  Both runs take their address from (frame, y, x)
// through the layout, so the second one lies one pitch (or one frame stride) further, not 3 w bytes; why its first k
// pixels -- left of that row, in padding or in the row above -- are inside the buffer: see px16 above.
template <class Src, bool BGR>
__global__ __launch_bounds__(256) void k_render_copy_to_rgb(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                            const int32_t *__restrict__ boxes, int n, int height, int width, int bh,
                                                            int bw, const uint8_t *in_end, const typename Src::lay L, const typename Src::colour KI,
                                                            const NoColour, const Packed) {
    const long long total_px = (long long)n * bh * bw, p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= total_px) return;
    const size_t fstride = L.template frame<Src>(height, width);
    const long long R = p0 / bw;
    const int col = (int)(p0 - R * bw);
    int f = (int)(R / bh), r = (int)(R - (long long)f * bh);
    int x0, y0;
    render_origin(boxes, f, height, width, bh, bw, x0, y0);
    uint32_t o[12];
    Src::template px16<BGR>(in + f * fstride, L, KI, height, width, y0 + r, x0 + col, in_end, o);
    const int k = bw - col;                                     // pixels of the group in row R
    if (k < 16 && p0 + k < total_px) {
        if (++r == bh) { r = 0; ++f; }
        render_origin(boxes, f, height, width, bh, bw, x0, y0);
        uint32_t o2[12];                                         // bytes [3k, 48) = the first pixels of the next row
        Src::template px16<BGR>(in + f * fstride, L, KI, height, width, y0 + r, x0 - k, in_end, o2);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int lim = 3 * k - 4 * i;                       // bytes of dword i that stay with row R
            const uint32_t m = lim >= 4 ? 0xffffffffu : lim <= 0 ? 0u : (1u << (8 * lim)) - 1u;
            o[i] = (o[i] & m) | (o2[i] & ~m);
        }
    }
    Src::template order16<BGR>(o);
    uint8_t *dst = out + p0 * 3;
    if (p0 + 16 <= total_px) {
        uint4 *d4 = (uint4 *)dst;
        d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
        d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
        d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
    } else {
        const int nb = (int)(total_px - p0) * 3;
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < nb) dst[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
    }
}

// The same to a pitched RGB output, whose rows are not one run: thread t owns pixels [16 g, 16 g + 16) of ONE output row (G =
// ceil(bw / 16) groups per row), one run through Src::px16 (the pixels right of the window are loaded -- inside the buffer or
// zero past its end, as for the NV12 kernel below -- and dropped).  Every row starts on 16 bytes (the launcher: out, frame_stride
// and pitch are multiples of 16), so a whole group is three aligned 16-byte stores; the last group of a row holds k = bw - 16 g
// < 16 pixels and stores exactly its 3 k bytes: the padding behind the row is never written.
template <class Src, bool BGR>
__global__ __launch_bounds__(256) void k_render_copy_to_rgb_rows(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                                 const int32_t *__restrict__ boxes, int n, int height, int width, int bh,
                                                                 int bw, const uint8_t *in_end, const typename Src::lay L,
                                                                 const typename Src::colour KI, const NoColour, const Pitched O) {
    const int G = (bw + 15) >> 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * bh * G) return;
    const long long R = t / G;
    const int g = (int)(t - R * G), f = (int)(R / bh), r = (int)(R - (long long)f * bh);
    int x0, y0;
    render_origin(boxes, f, height, width, bh, bw, x0, y0);
    uint32_t o[12];
    Src::template px16<BGR>(in + f * L.template frame<Src>(height, width), L, KI, height, width, y0 + r, x0 + 16 * g, in_end, o);
    Src::template order16<BGR>(o);
    uint8_t *dst = out + (size_t)f * (size_t)O.frame_stride + O.template rgb<size_t>(bw, r, 16 * g);
    const int k = bw - 16 * g;
    if (k >= 16) {
        uint4 *d4 = (uint4 *)dst;
        d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
        d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
        d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
    } else {
        const int nb = 3 * k;
#pragma unroll
        for (int i = 0; i < 48; ++i)
            if (i < nb) dst[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
    }
}

// --------------------------------------------------------------------------------------
// render to NV12 (no counterpart in the reference, whose renderer hands RGB / BGR to OpenCV's writer).  The RGB crop C of a
// frame is exactly what the RGB output is (same window rules, same clamping, the copy or the INTER_LINEAR
// resampling); the output frame u8 [oh * 3 / 2][ow] (oh, ow even) is C in the output's colour (Nv12Enc: BT.601 or BT.709,
// limited or full range; include/svc.h states the table), 20-bit fixed point, int32:
//   Y[y][x] = clamp((YR r + YG g + YB b + (Y0 << 20) + (1 << 19)) >> 20)
//   U[j][i] = clamp((UR sr + UG sg + UB sb + (128 << 22) + (1 << 21)) >> 22)      sr, sg, sb = sums over the 2 x 2 block
//   V[j][i] = clamp((VR sr + VG sg + VB sb + (128 << 22) + (1 << 21)) >> 22)      C[2j .. 2j+1][2i .. 2i+1]
// Limited range lands in 16..235 (Y) and 16..240 (U, V) for every input and the clamp never fires; full range reaches 256 in
// U for pure blue and in V for pure red, which the clamp makes 255.  Another matrix or range changes the constants only.
// NV12 in, NV12 out is the same thing on the converted crop; copying the planes of a native-size window at an even origin
// would give other bytes (and a picture that was never RGB) and is not done here.
// --------------------------------------------------------------------------------------
// (__mul24: the coefficients are below 2^23 in magnitude, the other factor at most 1020, the products fit 32 bits: exact.
// Every sum is positive (5.2e5 .. 1.074e9), so the shift is taken on the unsigned value -- the same number as the arithmetic
// one -- and the clamp has only its upper side.  Y needs none in any of the four colours (it ends in 0..255: the byte is
// masked, as it always was); U and V are cut at 2^30 - 1 BEFORE the shift, on the unsigned value: nothing here has the shape
// of the clamped shifts of nv12_rgb.)
__device__ __forceinline__ uint32_t rgb_luma(const Nv12Enc &K, uint32_t p) {                 // p = r | g << 8 | b << 16
    const int r = (int)(p & 0xffu), g = (int)((p >> 8) & 0xffu), b = (int)((p >> 16) & 0xffu);
    const int v = __mul24(K.yr, r) + __mul24(K.yg, g) + __mul24(K.yb, b) + K.yoff;
    return ((uint32_t)v >> 20) & 0xffu;
}
// the four pixels of a 2 x 2 block -> U | V << 8
__device__ __forceinline__ uint32_t rgb_chroma(const Nv12Enc &K, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
    // r and b summed in place (10-bit fields at bits 0 and 16), g on its own
    const uint32_t rb = (p0 & 0xff00ffu) + (p1 & 0xff00ffu) + (p2 & 0xff00ffu) + (p3 & 0xff00ffu);
    const int sr = (int)(rb & 0xffffu), sb = (int)(rb >> 16);
    const int sg = (int)(((p0 >> 8) & 0xffu) + ((p1 >> 8) & 0xffu) + ((p2 >> 8) & 0xffu) + ((p3 >> 8) & 0xffu));
    const int off = (128 << 22) + (1 << 21);
    const uint32_t top = (256u << 22) - 1u;
    const int u = __mul24(K.ur, sr) + __mul24(K.ug, sg) + __mul24(K.ub, sb) + off;
    const int v = __mul24(K.vr, sr) + __mul24(K.vg, sg) + __mul24(K.vb, sb) + off;
    return (min((uint32_t)u, top) >> 22) | ((min((uint32_t)v, top) >> 22) << 8);
}

// pixel i (a constant once unrolled) of the 48 bytes of a px16 run -> r | g << 8 | b << 16
__device__ __forceinline__ uint32_t run_px(const uint32_t (&o)[12], int i) {
    const int b = 3 * i, d = b >> 2;
    return __builtin_amdgcn_alignbyte(d + 1 < 12 ? o[d + 1] : 0u, o[d], b & 3) & 0xffffffu;
}

// 16 (or, half: the first 8) bytes to an 8-aligned address: one 16-byte store where the address allows it
__device__ __forceinline__ void st16_a8(uint8_t *d, const uint32_t (&v)[4], bool half) {
    if (half) *(uint2 *)d = make_uint2(v[0], v[1]);
    else if (((uintptr_t)d & 15) == 0) *(uint4 *)d = make_uint4(v[0], v[1], v[2], v[3]);
    else { *(uint2 *)d = make_uint2(v[0], v[1]); *(uint2 *)(d + 8) = make_uint2(v[2], v[3]); }
}

template <class OLay> struct DstNv12;
// To NV12, bw % 8 == 0, bw >= 16, every output row, luma or chroma, starting on 8 bytes (packed: out 16-aligned and that width;
// pitched: out, frame_stride, pitch, chroma_offset and chroma_pitch multiples of 8 -- DstNv12::vec_ok).
// Thread t owns the strip of window rows 2j, 2j + 1 by pixels [16 g, 16 g + 16) (the last strip of a row is 8 wide when
// bw % 16 == 8): two runs through Src::px16 (odd x, odd y and the frame's end are its business; the pixels past the window
// are converted and dropped), 32 luma bytes and the strip's 8 interleaved chroma pairs, each row of it as one aligned store.
template <class Src, class OLay>
__global__ __launch_bounds__(256) void k_render_copy_to_nv12(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                             const int32_t *__restrict__ boxes, int n, int height, int width, int bh,
                                                             int bw, const uint8_t *in_end, const typename Src::lay L, const typename Src::colour KI,
                                                             const Nv12Enc KO, const OLay O) {
    const int G = (bw + 15) >> 4, hb = bh >> 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * hb * G) return;
    const long long R = t / G;
    const int g = (int)(t - R * G), f = (int)(R / hb), j = (int)(R - (long long)f * hb);
    int x0, y0;
    render_origin(boxes, f, height, width, bh, bw, x0, y0);
    const uint8_t *fr = in + f * L.template frame<Src>(height, width);
    uint32_t a[12], b[12];
    Src::template px16<false>(fr, L, KI, height, width, y0 + 2 * j, x0 + 16 * g, in_end, a);
    Src::template px16<false>(fr, L, KI, height, width, y0 + 2 * j + 1, x0 + 16 * g, in_end, b);
    uint32_t ya[4] = {0u, 0u, 0u, 0u}, yb[4] = {0u, 0u, 0u, 0u}, uv[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) {                               // block i of the strip: pixels 2 i, 2 i + 1 of both rows
        const uint32_t p0 = run_px(a, 2 * i), p1 = run_px(a, 2 * i + 1), p2 = run_px(b, 2 * i), p3 = run_px(b, 2 * i + 1);
        ya[i >> 1] |= (rgb_luma(KO, p0) | (rgb_luma(KO, p1) << 8)) << (16 * (i & 1));
        yb[i >> 1] |= (rgb_luma(KO, p2) | (rgb_luma(KO, p3) << 8)) << (16 * (i & 1));
        uv[i >> 1] |= rgb_chroma(KO, p0, p1, p2, p3) << (16 * (i & 1));
    }
    uint8_t *o = out + f * O.template frame<DstNv12<OLay>>(bh, bw);
    const bool half = 16 * g + 16 > bw;
    st16_a8(o + O.template luma<size_t>(bw, 2 * j, 16 * g), ya, half);
    st16_a8(o + O.template luma<size_t>(bw, 2 * j + 1, 16 * g), yb, half);
    st16_a8(o + O.template chroma<size_t>(bh, bw, 2 * j, 16 * g), uv, half);
}

// --------------------------------------------------------------------------------------
// Pixel sinks: what the render kernels ask of an output format.  The crop is RGB (in the sink's channel order `bgr`) until
// a sink stores it.
//   size_ok, size_rule       the pictures the format can hold, and the words the error text says it with
//   flags_ok, flags_rule     the same for the SVC_RENDER_* flags
//   frame_bytes              bytes of one packed frame
//   olay                     the output layout OLay (`O`: the kernel's output-layout argument): every address of the output is the
//                            frame's start out + f * O.frame plus O.rgb / O.luma / O.chroma of the PICTURE's row and column
//                            (the RGB sink's row start: O.rgb_row, the same sum)
//   rows                     B: a thread of the per-pixel copy owns a B x B block of the crop, a resize workgroup B output rows
//   colour, col              the colour constants the sink converts with (a kernel argument, K below; NoColour for RGB) and
//                            the sink's part of a Colours pair
//   put_block                block (j, i) of the frame at `fo` from its pixels p[B * B] (row-major, as Src::px gives them)
//   vec_ok, vec_threads,     the copy path's vector kernel: the window widths, output addresses and layouts it takes (the frames
//   vec_copy<Src>            16-aligned besides), its threads, the kernel
//   lds_bytes                LDS of the resize kernel behind the two staged window rows
//   out_rows, dst_rows       the output rows that rows B j .. B j + B - 1 of the crop become (frame fy of `out`): how many, where
//   rgb_row                  where in that LDS row r of the workgroup's B rows is resampled to
//   rows_out                 the B resampled rows -> the output rows, by the whole workgroup (called behind a barrier)
// --------------------------------------------------------------------------------------
template <bool BGR, class OLay = Packed>
struct DstRgb {                                 // u8 [oh][ow][3]; Pitched: rows `pitch` bytes apart
    typedef OLay olay;
    typedef NoColour colour;
    static colour col(const Colours &) { return NoColour(); }
    static constexpr bool bgr = BGR;
    static constexpr int rows = 1;
    static bool size_ok(int oh, int ow) { return oh >= 1 && ow >= 1; }
    static const char *size_rule() { return "an RGB output has width and height >= 1"; }
    static bool flags_ok(int flags) { return !(flags & ~SVC_RENDER_BGR); }
    static const char *flags_rule() { return "flags has bits other than SVC_RENDER_BGR"; }
    __host__ __device__ static size_t frame_bytes(int oh, int ow) { return (size_t)oh * ow * 3; }
    // Packed: one run of pixels from a 16-aligned start; Pitched: every row starts on 16 bytes
    static bool vec_ok(const Packed &, const uint8_t *out, int bw) { return bw >= 16 && ((uintptr_t)out & 15) == 0; }
    static bool vec_ok(const Pitched &O, const uint8_t *out, int bw) {
        return bw >= 16 && (((uintptr_t)out | (uintptr_t)O.frame_stride | (uintptr_t)O.pitch) & 15) == 0;
    }
    static long long vec_threads(int n, int bh, int bw) {
        return std::is_same<OLay, Packed>::value ? ((long long)n * bh * bw + 15) / 16 : (long long)n * bh * ((bw + 15) / 16);
    }
    template <class Src>
    static auto vec_copy() {
        if constexpr (std::is_same<OLay, Packed>::value) return k_render_copy_to_rgb<Src, BGR>;
        else return k_render_copy_to_rgb_rows<Src, BGR>;
    }
    static size_t lds_bytes(int ow) { return (size_t)ow * 3 + 16; }

    __device__ __forceinline__ static void put_block(const colour &, const OLay &O, uint8_t *fo, int oh, int ow, int j, int i, const uint32_t (&p)[1]) {
        uint8_t *d = fo + O.template rgb<size_t>(ow, j, i);
        d[0] = (uint8_t)p[0];
        d[1] = (uint8_t)(p[0] >> 8);
        d[2] = (uint8_t)(p[0] >> 16);
    }
    // the row is resampled at the output row's own 16-byte phase and stored as it is
    static constexpr int out_rows = 1;
    __device__ __forceinline__ static void dst_rows(const OLay &O, uint8_t *out, int fy, int oh, int ow, int j, uint8_t *(&dst)[1]) {
        dst[0] = out + O.template rgb_row<size_t>(fy, oh, ow, j);
    }
    __device__ __forceinline__ static uint8_t *rgb_row(uint8_t *lds, uint8_t *const (&dst)[1], int ow, int r) {
        return lds + (int)((uintptr_t)dst[0] & 15);
    }
    __device__ __forceinline__ static void rows_out(const colour &, uint8_t *lds, uint8_t *const (&dst)[1], int ow) {
        row_out(dst[0], rgb_row(lds, dst, ow, 0), ow * 3);
    }
};

template <class OLay = Packed>
struct DstNv12 {                                // u8 [oh * 3 / 2][ow], the formula above; Pitched: as SrcNv12's
    typedef OLay olay;
    typedef Nv12Enc colour;
    static colour col(const Colours &c) { return c.enc; }
    static constexpr bool bgr = false;
    static constexpr int rows = 2;
    static bool size_ok(int oh, int ow) { return oh >= 2 && ow >= 2 && !(oh & 1) && !(ow & 1); }
    static const char *size_rule() {
        return "width and height of an NV12 output are even and >= 2; a window of odd size needs an even output size";
    }
    static bool flags_ok(int flags) { return flags == 0; }
    static const char *flags_rule() { return "flags must be 0 (SVC_RENDER_BGR has no meaning for an NV12 output)"; }
    __host__ __device__ static size_t frame_bytes(int oh, int ow) { return (size_t)(oh + (oh >> 1)) * ow; }
    // st16_a8 needs every luma and chroma row start on 8 bytes (the packed path keeps the 16-aligned out it has always asked for)
    static bool vec_ok(const Packed &, const uint8_t *out, int bw) { return bw >= 16 && bw % 8 == 0 && ((uintptr_t)out & 15) == 0; }
    static bool vec_ok(const Pitched &O, const uint8_t *out, int bw) {
        return bw >= 16 && bw % 8 == 0 &&
               (((uintptr_t)out | (uintptr_t)O.frame_stride | (uintptr_t)O.pitch | (uintptr_t)O.chroma_offset | (uintptr_t)O.chroma_pitch) & 7) == 0;
    }
    static long long vec_threads(int n, int bh, int bw) { return (long long)n * (bh / 2) * ((bw + 15) / 16); }
    template <class Src>
    static auto vec_copy() { return k_render_copy_to_nv12<Src, OLay>; }
    // two RGB rows of rgb_cap bytes, then three output rows (two of luma, one of chroma) of row_cap bytes
    __host__ __device__ static int rgb_cap(int ow) { return (ow * 3 + 15) / 16 * 16; }
    __host__ __device__ static int row_cap(int ow) { return (ow + 15) / 16 * 16 + 16; }
    static size_t lds_bytes(int ow) { return 2 * (size_t)rgb_cap(ow) + 3 * (size_t)row_cap(ow); }

    __device__ __forceinline__ static void put_block(const colour &K, const OLay &O, uint8_t *fo, int oh, int ow, int j, int i, const uint32_t (&p)[4]) {
        uint8_t *d0 = fo + O.template luma<size_t>(ow, 2 * j, 2 * i), *d1 = fo + O.template luma<size_t>(ow, 2 * j + 1, 2 * i);
        uint8_t *dc = fo + O.template chroma<size_t>(oh, ow, 2 * j, 2 * i);
        const uint32_t c = rgb_chroma(K, p[0], p[1], p[2], p[3]);
        d0[0] = (uint8_t)rgb_luma(K, p[0]);
        d0[1] = (uint8_t)rgb_luma(K, p[1]);
        d1[0] = (uint8_t)rgb_luma(K, p[2]);
        d1[1] = (uint8_t)rgb_luma(K, p[3]);
        dc[0] = (uint8_t)c;
        dc[1] = (uint8_t)(c >> 8);
    }
    static constexpr int out_rows = 3;
    __device__ __forceinline__ static void dst_rows(const OLay &O, uint8_t *out, int fy, int oh, int ow, int j, uint8_t *(&dst)[3]) {
        uint8_t *fo = out + fy * O.template frame<DstNv12>(oh, ow);
        dst[0] = fo + O.template luma<size_t>(ow, 2 * j, 0);
        dst[1] = fo + O.template luma<size_t>(ow, 2 * j + 1, 0);
        dst[2] = fo + O.template chroma<size_t>(oh, ow, 2 * j, 0);
    }
    __device__ __forceinline__ static uint8_t *rgb_row(uint8_t *lds, uint8_t *const (&dst)[3], int ow, int r) {
        return lds + r * rgb_cap(ow);
    }
    // every 2 x 2 block of the two RGB rows is converted into the three output rows, each at the 16-byte phase of its
    // place in the output
    __device__ __forceinline__ static void rows_out(const colour &K, uint8_t *lds, uint8_t *const (&dst)[3], int ow) {
        const int cap = rgb_cap(ow);
        uint8_t *lrow[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) lrow[k] = lds + 2 * cap + k * row_cap(ow) + (int)((uintptr_t)dst[k] & 15);
        for (int i = threadIdx.x; 2 * i < ow; i += 256) {
            const uint8_t *s0 = lds + 6 * i, *s1 = s0 + cap;
            const uint32_t p0 = s0[0] | (s0[1] << 8) | (s0[2] << 16), p1 = s0[3] | (s0[4] << 8) | (s0[5] << 16);
            const uint32_t p2 = s1[0] | (s1[1] << 8) | (s1[2] << 16), p3 = s1[3] | (s1[4] << 8) | (s1[5] << 16);
            const uint32_t c = rgb_chroma(K, p0, p1, p2, p3);
            lrow[0][2 * i] = (uint8_t)rgb_luma(K, p0);
            lrow[0][2 * i + 1] = (uint8_t)rgb_luma(K, p1);
            lrow[1][2 * i] = (uint8_t)rgb_luma(K, p2);
            lrow[1][2 * i + 1] = (uint8_t)rgb_luma(K, p3);
            lrow[2][2 * i] = (uint8_t)c;
            lrow[2][2 * i + 1] = (uint8_t)(c >> 8);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k) row_out(dst[k], lrow[k], ow);
    }
};

// Copy path for everything the vector kernels leave (narrow windows, other widths, unaligned buffers): one thread per
// B x B block of the crop (B = Dst::rows), byte accesses.
template <class Src, class Dst>
__global__ __launch_bounds__(256) void k_render_copy_px(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                        const int32_t *__restrict__ boxes, int height, int width, int bh, int bw,
                                                        long long total, const typename Src::lay L, const typename Src::colour KI,
                                                        const typename Dst::colour KO, const typename Dst::olay O) {
    constexpr int B = Dst::rows;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int wb = bw / B, hb = bh / B;
    const long long R = t / wb;
    const int i = (int)(t - R * wb), f = (int)(R / hb), j = (int)(R - (long long)f * hb);
    int x0, y0;
    render_origin(boxes, f, height, width, bh, bw, x0, y0);
    const uint8_t *fr = in + f * L.template frame<Src>(height, width);
    uint32_t p[B * B];
#pragma unroll
    for (int k = 0; k < B * B; ++k) p[k] = Src::template px<Dst::bgr>(fr, L, KI, height, width, y0 + B * j + k / B, x0 + B * i + k % B);
    Dst::put_block(KO, O, out + f * O.template frame<Dst>(bh, bw), bh, bw, j, i, p);
}

// Resize path: k_cv_resize's arithmetic on a window of the full frame.  One workgroup = B output rows of one frame (B =
// Dst::rows).  Per row, the two window rows it reads are staged in LDS as RGB (Src::stage_row; R and B are swapped only on
// the way out of them) and resampled into the LDS row the sink names; then the sink stores its rows with aligned 16-byte
// stores (row_out).  LDS: two source rows of span_cap bytes, then Dst::lds_bytes.
// (amdgpu_num_sgpr: 256-thread blocks are resident 8 | 7 | 6 per CU at <= 80 | <= 96 | more scalar registers, which the compiler
// does not count as a cost; the NV12 sink's colour constants, live from the kernel's entry, would take it from 96 to 106)
template <class Src, class Dst>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void k_render_resize(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                       const int *__restrict__ tab, const int32_t *__restrict__ boxes, int f0,
                                                       int height, int width, int bh, int bw, int oh, int ow, int span_cap,
                                                       const uint8_t *in_end, int vec, const typename Src::lay L, const typename Src::colour KI,
                                                       const typename Dst::colour KO, const typename Dst::olay O) {
    extern __shared__ __align__(16) uint8_t sm_rr[];
    const CvLinear T(tab, oh, ow);
    const int j = blockIdx.x, f = f0 + blockIdx.y;
    int x0, y0;
    render_origin(boxes, f, height, width, bh, bw, x0, y0);
    const uint8_t *fr = in + f * L.template frame<Src>(height, width);
    uint8_t *lds = sm_rr + 2 * span_cap, *dst[Dst::out_rows];
    for (int r = 0; r < Dst::rows; ++r) {
        int ry[2], b0, b1, sh[2];
        T.row(Dst::rows * j + r, bh, ry[0], ry[1], b0, b1);
        if (r) __syncthreads();                                 // row 0's resampling has read the staged rows
#pragma unroll
        for (int k = 0; k < 2; ++k)
            sh[k] = Src::stage_row(fr, L, KI, height, width, y0 + ry[k], x0, bw, sm_rr + k * span_cap, span_cap, in_end, vec);
        if (!r) Dst::dst_rows(O, out, blockIdx.y, oh, ow, j, dst);
        uint8_t *orow = Dst::rgb_row(lds, dst, ow, r);
        __syncthreads();
        const uint8_t *r0 = sm_rr + sh[0], *r1 = sm_rr + span_cap + sh[1];
        for (int ox = threadIdx.x; ox < ow; ox += 256) {
            int sx, sx1, a0, a1;
            bool inner;
            T.col(ox, bw, sx, sx1, a0, a1, inner);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                orow[ox * 3 + (Dst::bgr ? 2 - c : c)] = CvLinear::blend(r0[sx * 3 + c], r0[sx1 * 3 + c], r1[sx * 3 + c], r1[sx1 * 3 + c],
                                                                        a0, a1, b0, b1, inner);
        }
    }
    __syncthreads();
    Dst::rows_out(KO, lds, dst, ow);
}

// Sub-pixel windows (svc_render_windows_q8; no counterpart in the reference, whose windows start on whole pixels): k_render_resize
// with the window's top-left corner given in 1/256 pixel.  The origin is clamped to [0, (width - bw) * 256] x [0, (height - bh) *
// 256] and split into a whole pixel (xi, yi) and a phase (xf, yf); a zero phase keeps the table's taps and weights, and a phase
// above zero moves the position the table gives -- tap * 2048 + the 11-bit weight of the far tap, the fraction zero where the
// table clamped it at the window's edge -- by 8 * phase, i.e. by phase / 256 pixel in units of 1 / 2048.  The position stays
// <= bw - 1 (bh - 1), and a phase above zero means xi < width - bw (yi < height - bh), so the far tap xi + bw (yi + bh) is a
// pixel of the frame; with a zero phase it is not tapped, and staged only where the frame has it.  Integers only; nothing is
// built per call.
__device__ __forceinline__ void render_origin_q8(const int32_t *__restrict__ origins, int f, int height, int width, int bh, int bw,
                                                 int &xi, int &xf, int &yi, int &yf) {
    const int X = (int)min(max((long long)origins[2 * f], 0ll), (long long)(width - bw) * 256);
    const int Y = (int)min(max((long long)origins[2 * f + 1], 0ll), (long long)(height - bh) * 256);
    xi = X >> 8; xf = X & 255;
    yi = Y >> 8; yf = Y & 255;
}

// The structure, the sources, the sinks and the register cap are k_render_resize's.  What differs: the origin and the phases are
// read once per workgroup (wave-uniform), a staged row holds min(bw + 1, width - xi) columns (the far column only where the
// frame has it), and every row and column derives its taps from the shared table with a multiply-add, a shift and a mask.
// LDS: two source rows of span_cap = 3 (bw + 1) + 32 (rounded up to 16) bytes, then Dst::lds_bytes.
template <class Src, class Dst>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(96))) void k_render_resize_q8(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                       const int *__restrict__ tab, const int32_t *__restrict__ origins, int f0,
                                                       int height, int width, int bh, int bw, int oh, int ow, int span_cap,
                                                       const uint8_t *in_end, int vec, const typename Src::lay L, const typename Src::colour KI,
                                                       const typename Dst::colour KO, const typename Dst::olay O) {
    extern __shared__ __align__(16) uint8_t sm_rq[];
    const CvLinear T(tab, oh, ow);
    const int j = blockIdx.x, f = f0 + blockIdx.y;
    int xi, xf, yi, yf;
    render_origin_q8(origins, f, height, width, bh, bw, xi, xf, yi, yf);
    const int ncols = min(bw + 1, width - xi);
    const uint8_t *fr = in + f * L.template frame<Src>(height, width);
    uint8_t *lds = sm_rq + 2 * span_cap, *dst[Dst::out_rows];
    for (int r = 0; r < Dst::rows; ++r) {
        int ry[2], b0, b1, sh[2];
        T.row(Dst::rows * j + r, bh, ry[0], ry[1], b0, b1);
        if (yf) {                                               // (both rows clamped to one: the table's position is that row)
            const int q = ry[0] * 2048 + (ry[1] > ry[0] ? b1 : 0) + 8 * yf;
            ry[0] = q >> 11;
            ry[1] = ry[0] + 1;                                  // <= bh, and yi + bh is a row of the frame
            b1 = q & 2047;
            b0 = 2048 - b1;
        }
        if (r) __syncthreads();                                 // row 0's resampling has read the staged rows
#pragma unroll
        for (int k = 0; k < 2; ++k)
            sh[k] = Src::stage_row(fr, L, KI, height, width, yi + ry[k], xi, ncols, sm_rq + k * span_cap, span_cap, in_end, vec);
        if (!r) Dst::dst_rows(O, out, blockIdx.y, oh, ow, j, dst);
        uint8_t *orow = Dst::rgb_row(lds, dst, ow, r);
        __syncthreads();
        const uint8_t *r0 = sm_rq + sh[0], *r1 = sm_rq + span_cap + sh[1];
        for (int ox = threadIdx.x; ox < ow; ox += 256) {
            int sx, sx1, a0, a1;
            bool inner;
            T.col(ox, bw, sx, sx1, a0, a1, inner);
            // selects on the wave-uniform phase, not a branch; xf > 0: sx1 <= bw = ncols - 1
            const int p = sx * 2048 + a1 + 8 * xf, ps = p >> 11, pa = p & 2047;
            sx = xf ? ps : sx;
            sx1 = xf ? ps + 1 : sx1;
            a1 = xf ? pa : a1;
            a0 = xf ? 2048 - pa : a0;
            // every column blends both taps: from xmax on the table holds sx = bw - 1, a0 = 2048 and a1 = 0 exactly (its fraction is
            // set to zero there), so t00 * a0 + t01 * a1 IS the plain copy t00 * 2048 of the integer kernel, without its per-lane branch
#pragma unroll
            for (int c = 0; c < 3; ++c)
                orow[ox * 3 + (Dst::bgr ? 2 - c : c)] = CvLinear::blend(r0[sx * 3 + c], r0[sx1 * 3 + c], r1[sx * 3 + c], r1[sx1 * 3 + c],
                                                                        a0, a1, b0, b1, true);
        }
    }
    __syncthreads();
    Dst::rows_out(KO, lds, dst, ow);
}

// --------------------------------------------------------------------------------------
// The renderer's host layer (the file's header names its parts)
// --------------------------------------------------------------------------------------
struct RenderCall {                         // what a render call is, whichever entry it came through; the layouts are types and travel beside it
    const char *name;                       // the entry the errors are reported under
    SvcHandle *h;
    const uint8_t *frames;
    int n, height, width;
    const int32_t *win;                     // the frames' windows: int32 [n][4] boxes; render_windows: [n][2] origins in 1/256 pixel
    int bw, bh;
    uint8_t *out;
    int oh, ow, flags;
    void *stream;
    Colours C;                              // of both sides, checked
};

// What the launchers share, around the two parts each keeps.  The argument checks: plain comparisons, before any device work.
// Then `rule`, the launcher's host half (its LDS rule, the host side of its tables), which may refuse the call; n = 0 is a no-op
// from there on.  Then the device, and `launch` with what guards the kernels' 16-byte loads -- the end of the last frame's last
// plane row (Packed: frames + n * frame_bytes) and whether they may run at all -- and the stream.
template <class Src, class Dst, class Rule, class Launch>
static int render_run(const RenderCall &c, const typename Src::lay &L, Rule rule, Launch launch) {
    if (!c.h || c.n < 0 || (c.n > 0 && (!c.frames || !c.win || !c.out)) || !Src::size_ok(c.height, c.width) || c.bw < 1 || c.bh < 1 ||
        c.bw > c.width || c.bh > c.height) {                                               // n = 0: a no-op, null buffers allowed
        svc_set_error("%s: invalid argument%s", c.name, Src::size_rule());
        return SVC_E_INVALID;
    }
    if (!Dst::size_ok(c.oh, c.ow)) {
        svc_set_error("%s: an output of %dx%d (%s)", c.name, c.ow, c.oh, Dst::size_rule());
        return SVC_E_INVALID;
    }
    if (!Dst::flags_ok(c.flags)) {
        svc_set_error("%s: %s", c.name, Dst::flags_rule());
        return SVC_E_INVALID;
    }
    const int rc = rule();
    if (rc || c.n == 0) return rc;
    SVC_HIP(hipSetDevice(c.h->device));
    const uint8_t *in_end = c.frames + (size_t)(c.n - 1) * L.template frame<Src>(c.height, c.width) + Src::extent(L, c.height, c.width);
    const bool vec = ((uintptr_t)c.frames & 15) == 0 && Src::vec_ok(L);
    return launch(in_end, vec, (hipStream_t)c.stream);
}

template <class Dst>
static int lds_refused(const RenderCall &c, const char *filter, size_t lds) {
    svc_set_error("%s: window %dx%d -> %dx%d%s needs %zu bytes of LDS per %s (> 64 KiB)", c.name, c.bw, c.bh, c.ow, c.oh, filter, lds,
                  Dst::rows == 1 ? "output row" : "pair of output rows");
    return SVC_E_INVALID;
}

// The linear launcher: the copy kernels at oh == bh && ow == bw (no LDS rule there), else k_render_resize.
template <class Src, class Dst>
static int render_crops(const RenderCall &c, const typename Src::lay &L, const typename Dst::olay &O) {
    const bool copy = c.oh == c.bh && c.ow == c.bw;
    int span_cap = 0;           // (set by the rule, read by the launch)
    size_t lds = 0;
    return render_run<Src, Dst>(c, L,
        [&] {
            span_cap = (c.bw * 3 + 32 + 15) / 16 * 16;
            lds = 2 * (size_t)span_cap + Dst::lds_bytes(c.ow);
            return !copy && lds > 65536 ? lds_refused<Dst>(c, "", lds) : SVC_OK;
        },
        [&](const uint8_t *in_end, bool vec, hipStream_t s) {
            const int *tab = nullptr;
            if (int rc = copy ? SVC_OK : cv_tab(c.h, c.bh, c.bw, c.oh, c.ow, &tab)) return rc;
            ProfScope ps(c.h, SVC_K_RENDER, s);
            if (copy) {
                if (vec && Dst::vec_ok(O, c.out, c.bw)) {          // (the layout decides which path runs, never whether the call is legal)
                    const unsigned grid = (unsigned)((Dst::vec_threads(c.n, c.bh, c.bw) + 255) / 256);
                    Dst::template vec_copy<Src>()<<<grid, 256, 0, s>>>(c.frames, c.out, c.win, c.n, c.height, c.width, c.bh, c.bw, in_end, L,
                                                                       Src::col(c.C), Dst::col(c.C), O);
                } else {
                    const long long total = (long long)c.n * (c.bh / Dst::rows) * (c.bw / Dst::rows);
                    k_render_copy_px<Src, Dst><<<(unsigned)((total + 255) / 256), 256, 0, s>>>(c.frames, c.out, c.win, c.height, c.width, c.bh, c.bw,
                                                                                               total, L, Src::col(c.C), Dst::col(c.C), O);
                }
                SVC_CHECK_LAUNCH();
                return SVC_OK;
            }
            for (int f0 = 0; f0 < c.n; f0 += 65535) {            // grid y <= 65535 frames per launch
                const dim3 grid((unsigned)(c.oh / Dst::rows), (unsigned)std::min(c.n - f0, 65535));
                k_render_resize<Src, Dst><<<grid, 256, lds, s>>>(c.frames, c.out + f0 * O.template frame<Dst>(c.oh, c.ow), tab, c.win, f0, c.height,
                                                                 c.width, c.bh, c.bw, c.oh, c.ow, span_cap, in_end, vec, L, Src::col(c.C),
                                                                 Dst::col(c.C), O);
                SVC_CHECK_LAUNCH();
            }
            return SVC_OK;
        });
}

// The launcher for windows whose origins are given in 1/256 pixel (svc_render_windows_q8): always the resampling kernel, also at
// oh == bh && ow == bw (the identity table: a pure fractional shift), with one more staged column in the LDS rule.
template <class Src, class Dst>
static int render_windows(const RenderCall &c, const typename Src::lay &L, const typename Dst::olay &O) {
    int span_cap = 0;           // (set by the rule, read by the launch)
    size_t lds = 0;
    return render_run<Src, Dst>(c, L,
        [&] {
            span_cap = ((c.bw + 1) * 3 + 32 + 15) / 16 * 16;
            lds = 2 * (size_t)span_cap + Dst::lds_bytes(c.ow);
            return lds > 65536 ? lds_refused<Dst>(c, "", lds) : SVC_OK;
        },
        [&](const uint8_t *in_end, bool vec, hipStream_t s) {
            const int *tab = nullptr;
            if (int rc = cv_tab(c.h, c.bh, c.bw, c.oh, c.ow, &tab)) return rc;
            ProfScope ps(c.h, SVC_K_RENDER, s);
            for (int f0 = 0; f0 < c.n; f0 += 65535) {            // grid y <= 65535 frames per launch
                const dim3 grid((unsigned)(c.oh / Dst::rows), (unsigned)std::min(c.n - f0, 65535));
                k_render_resize_q8<Src, Dst><<<grid, 256, lds, s>>>(c.frames, c.out + f0 * O.template frame<Dst>(c.oh, c.ow), tab, c.win, f0,
                                                                    c.height, c.width, c.bh, c.bw, c.oh, c.ow, span_cap, in_end, vec, L,
                                                                    Src::col(c.C), Dst::col(c.C), O);
                SVC_CHECK_LAUNCH();
            }
            return SVC_OK;
        });
}

// --------------------------------------------------------------------------------------
// Lanczos path: PIL.Image.resize(LANCZOS) of the window (Pillow's two 8-bit fixed-point passes, svc_lanczos.h builds its tables;
// no counterpart in the reference, which never resamples its crops).  One workgroup = one frame x a band of B output rows (B a
// multiple of Dst::rows).  From the vertical bounds it takes the window rows [r_lo, r_hi) that the band's filters touch, stages
// them LZ_STAGE at a time as RGB bytes (Src::stage_row, as k_render_resize does: NV12 is converted there), resamples every
// staged row horizontally ONCE into the LDS tile T[r_hi - r_lo][3 ow] u8 (the u8 intermediate of Pillow's two passes; nothing of
// it goes to global memory), then runs the vertical pass from the tile into the sink's LDS rows, Dst::rows of them at a time,
// and lets the sink store them (Dst::rows_out).  The filters are cut at the window's edge because the tables are those of a
// bw x bh picture: a pixel outside the window is never staged.  A pass whose sizes are equal runs on lanczos_tab's identity
// table (one tap of 1 << 22: the value itself).  Integer arithmetic only: int32 accumulators from 1 << 21, products by
// __mul24 (the launcher checked |coefficient| < 2^23), arithmetic shift by 22, clamp to 0..255.
// LDS: LZ_STAGE rows of span_cap bytes | tile_cap rows of tw = 3 ow rounded up to 16 bytes | Dst::lds_bytes(ow).
// The horizontal tables are read from global memory (every workgroup reads the same few KB: L2 / L1 hits); the vertical
// coefficients of an output row are the same for the whole workgroup.
// --------------------------------------------------------------------------------------
#define LZ_STAGE 2

// clamp(acc >> 22, 0, 255), taken as clamp(acc, 0, 2^30 - 1) >> 22 for the reason given at nv12_rgb
__device__ __forceinline__ uint8_t lz_u8(int acc) { return (uint8_t)(min(max(acc, 0), (256 << LZ_PREC) - 1) >> LZ_PREC); }

template <class Src, class Dst>
__global__ __launch_bounds__(256) void k_render_lanczos(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                        const int *__restrict__ hb, const int *__restrict__ hk, int hks,
                                                        const int *__restrict__ vb, const int *__restrict__ vk, int vks,
                                                        const int32_t *__restrict__ boxes, int f0, int height, int width, int bh,
                                                        int bw, int oh, int ow, int B, int span_cap, int tile_cap,
                                                        const uint8_t *in_end, int vec, const typename Src::lay L, const typename Src::colour KI,
                                                        const typename Dst::colour KO, const typename Dst::olay O) {
    extern __shared__ __align__(16) uint8_t sm_lz[];
    const int tw = (ow * 3 + 15) / 16 * 16;
    uint8_t *tile = sm_lz + LZ_STAGE * span_cap, *lds = tile + tile_cap * tw;
    const int f = f0 + blockIdx.y, oy0 = blockIdx.x * B, oy1 = min(oh, oy0 + B);
    int x0, y0;
    render_origin(boxes, f, height, width, bh, bw, x0, y0);
    const uint8_t *fr = in + f * L.template frame<Src>(height, width);
    const int r_lo = vb[2 * oy0], nr = min(vb[2 * (oy1 - 1)] + vb[2 * (oy1 - 1) + 1] - r_lo, tile_cap);

    // horizontal pass: window rows r_lo + r .. -> tile rows r ..; a thread owns output columns, three channels of LZ_STAGE rows
    for (int r = 0; r < nr; r += LZ_STAGE) {
        if (r) __syncthreads();                                 // the rows staged before have been resampled
        int sh[LZ_STAGE];
#pragma unroll
        for (int s = 0; s < LZ_STAGE; ++s)                      // (r + s < nr is the same for the whole workgroup)
            sh[s] = r + s < nr ? Src::stage_row(fr, L, KI, height, width, y0 + r_lo + r + s, x0, bw, sm_lz + s * span_cap, span_cap, in_end, vec) : 0;
        __syncthreads();
        for (int ox = threadIdx.x; ox < ow; ox += 256) {
            const int xmin = hb[2 * ox], cnt = hb[2 * ox + 1];
            const int *k = hk + (size_t)ox * hks;
            int acc[LZ_STAGE][3];
#pragma unroll
            for (int s = 0; s < LZ_STAGE; ++s)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[s][c] = 1 << (LZ_PREC - 1);
            for (int j = 0; j < cnt; ++j) {
                const int kj = k[j];
#pragma unroll
                for (int s = 0; s < LZ_STAGE; ++s) {            // (a row past nr: whatever the staging row holds, never stored)
                    const uint8_t *p = sm_lz + s * span_cap + sh[s] + (xmin + j) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) acc[s][c] += __mul24((int)p[c], kj);
                }
            }
#pragma unroll
            for (int s = 0; s < LZ_STAGE; ++s)
                if (r + s < nr) {
                    uint8_t *t = tile + (r + s) * tw + ox * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) t[c] = lz_u8(acc[s][c]);
                }
        }
    }
    __syncthreads();

    // vertical pass: a thread owns four consecutive bytes of the output row (one dword of every tile row it taps)
    const int nb = ow * 3, nd = (nb + 3) >> 2, tw4 = tw >> 2;
    uint8_t *dst[Dst::out_rows];
    for (int oy = oy0; oy < oy1; oy += Dst::rows) {
        if (oy > oy0) __syncthreads();                          // the sink has stored the rows before
        Dst::dst_rows(O, out, blockIdx.y, oh, ow, oy / Dst::rows, dst);
#pragma unroll
        for (int r = 0; r < Dst::rows; ++r) {
            const int ymin = vb[2 * (oy + r)], cnt = vb[2 * (oy + r) + 1];
            const int *k = vk + (size_t)(oy + r) * vks;
            const uint32_t *t = (const uint32_t *)(tile + (ymin - r_lo) * tw);
            uint8_t *orow = Dst::rgb_row(lds, dst, ow, r);
            for (int d = threadIdx.x; d < nd; d += 256) {
                int acc[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = 1 << (LZ_PREC - 1);
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t v = t[j * tw4 + d];
                    const int kj = k[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += __mul24((int)((v >> (8 * e)) & 0xffu), kj);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int b = 4 * d + e, c = b % 3;
                    if (b < nb) orow[Dst::bgr ? b + 2 - 2 * c : b] = lz_u8(acc[e]);      // R and B swapped on the way out
                }
            }
        }
        __syncthreads();
        Dst::rows_out(KO, lds, dst, ow);
    }
}

// The LANCZOS table of one axis, in -> out, built once per handle and size pair and checked on the host:
//   every |coefficient| < 2^23                 __mul24 is exact
//   255 * sum |coefficient| + 2^21 < 2^31      no accumulator leaves int32 (Pillow's own range)
static int lz_tab(const char *name, SvcHandle *h, int in_size, int out_size, ResampleTab **out) {
    auto key = std::make_pair(in_size, out_size);
    auto it = h->lztabs.find(key);
    if (it == h->lztabs.end()) {
        ResampleTab t;
        lanczos_tab(in_size, out_size, t.bounds_host, t.coeff_host, t.ksize);
        for (int i = 0; i < out_size; ++i) {
            long long sum = 0;
            for (int j = 0; j < t.ksize; ++j) {
                const long long c = std::abs((long long)t.coeff_host[(size_t)i * t.ksize + j]);
                if (c >= (1ll << 23)) {
                    svc_set_error("%s: LANCZOS table %d -> %d has a coefficient of magnitude %lld (>= 2^23)", name, in_size, out_size, c);
                    return SVC_E_INVALID;
                }
                sum += c;
            }
            if (255 * sum + (1ll << (LZ_PREC - 1)) >= (1ll << 31)) {
                svc_set_error("%s: LANCZOS table %d -> %d: 255 * %lld + 2^21 leaves int32", name, in_size, out_size, sum);
                return SVC_E_INVALID;
            }
        }
        it = h->lztabs.emplace(key, std::move(t)).first;
    }
    *out = &it->second;
    return SVC_OK;
}
static int lz_upload(ResampleTab &t) {
    if (t.coeff.p) return SVC_OK;
    int rc = t.bounds.ensure(t.bounds_host.size() * 4);
    if (rc) return rc;
    SVC_HIP(hipMemcpy(t.bounds.p, t.bounds_host.data(), t.bounds_host.size() * 4, hipMemcpyHostToDevice));
    DevBuf c;
    rc = c.ensure(t.coeff_host.size() * 4);
    if (rc) return rc;
    SVC_HIP(hipMemcpy(c.p, t.coeff_host.data(), t.coeff_host.size() * 4, hipMemcpyHostToDevice));
    t.coeff = std::move(c);
    std::vector<int>().swap(t.coeff_host);
    return SVC_OK;
}

// the most window rows a band of B output rows touches (the tile's height), from the vertical bounds
static int lz_tile_rows(const std::vector<int> &vb, int oh, int B) {
    int cap = 0;
    for (int y0 = 0; y0 < oh; y0 += B) {
        int lo = INT32_MAX, hi = 0;
        for (int y = y0; y < std::min(oh, y0 + B); ++y) {
            lo = std::min(lo, vb[2 * y]);
            hi = std::max(hi, vb[2 * y] + vb[2 * y + 1]);
        }
        cap = std::max(cap, hi - lo);
    }
    return cap;
}

// The Lanczos launcher.  oh == bh && ow == bw skips both passes: the linear launcher's exact copy (whose argument checks are
// these).  The band: the largest B <= 32 (a multiple of Dst::rows) whose LDS fits in 64 KiB (include/svc.h states the formula).
template <class Src, class Dst>
static int render_crops_lanczos(const RenderCall &c, const typename Src::lay &L, const typename Dst::olay &O) {
    if (c.oh == c.bh && c.ow == c.bw) return render_crops<Src, Dst>(c, L, O);
    ResampleTab *ht = nullptr, *vt = nullptr;
    int span_cap = 0, B = 0, tile_cap = 0;
    size_t lds = 0;
    return render_run<Src, Dst>(c, L,
        [&] {
            int rc;
            if ((rc = lz_tab(c.name, c.h, c.bw, c.ow, &ht)) || (rc = lz_tab(c.name, c.h, c.bh, c.oh, &vt))) return rc;
            span_cap = (c.bw * 3 + 32 + 15) / 16 * 16;
            const int tw = (c.ow * 3 + 15) / 16 * 16;
            const size_t fixed = (size_t)LZ_STAGE * span_cap + Dst::lds_bytes(c.ow);
            for (B = std::min(32, (c.oh + Dst::rows - 1) / Dst::rows * Dst::rows) / Dst::rows * Dst::rows;; B -= Dst::rows) {
                tile_cap = lz_tile_rows(vt->bounds_host, c.oh, B);
                lds = fixed + (size_t)tile_cap * tw;
                if (lds <= 65536) return SVC_OK;
                if (B == Dst::rows) return lds_refused<Dst>(c, " (lanczos)", lds);
            }
        },
        [&](const uint8_t *in_end, bool vec, hipStream_t s) {
            for (ResampleTab *t : {ht, vt}) if (int rc = lz_upload(*t)) return rc;
            ProfScope ps(c.h, SVC_K_RENDER, s);
            for (int f0 = 0; f0 < c.n; f0 += 65535) {            // grid y <= 65535 frames per launch
                const dim3 grid((unsigned)((c.oh + B - 1) / B), (unsigned)std::min(c.n - f0, 65535));
                k_render_lanczos<Src, Dst><<<grid, 256, lds, s>>>(c.frames, c.out + f0 * O.template frame<Dst>(c.oh, c.ow), (const int *)ht->bounds.p,
                                                                  (const int *)ht->coeff.p, ht->ksize, (const int *)vt->bounds.p,
                                                                  (const int *)vt->coeff.p, vt->ksize, c.win, f0, c.height, c.width, c.bh, c.bw,
                                                                  c.oh, c.ow, B, span_cap, tile_cap, in_end, vec, L, Src::col(c.C), Dst::col(c.C), O);
                SVC_CHECK_LAUNCH();
            }
            return SVC_OK;
        });
}

// The source x sink pairings of one source layout and one output layout, stated once: f is called with a Pair of the kernels'
// Src and Dst for the frames' format, the output's format and (flags) the RGB sink's channel order.
template <class S, class D> struct Pair { typedef S Src; typedef D Dst; };
template <class Lay, class OLay, class F>
static int render_pair(int pix_fmt, bool to_nv12, int flags, F f) {
    const bool nv12 = pix_fmt == SVC_FMT_NV12;
    if (to_nv12) return nv12 ? f(Pair<SrcNv12<Lay>, DstNv12<OLay>>()) : f(Pair<SrcRgb<Lay>, DstNv12<OLay>>());
    if (flags & SVC_RENDER_BGR) return nv12 ? f(Pair<SrcNv12<Lay>, DstRgb<true, OLay>>()) : f(Pair<SrcRgb<Lay>, DstRgb<true, OLay>>());
    return nv12 ? f(Pair<SrcNv12<Lay>, DstRgb<false, OLay>>()) : f(Pair<SrcRgb<Lay>, DstRgb<false, OLay>>());
}

// The four packed entries: the linear launcher on the Packed policies of both sides (the measured default path), BT.601 limited.
static int render_crops_packed(const RenderCall &c, int pix_fmt, bool to_nv12) {
    return render_pair<Packed, Packed>(pix_fmt, to_nv12, c.flags, [&](auto p) {
        return render_crops<typename decltype(p)::Src, typename decltype(p)::Dst>(c, Packed(), Packed());
    });
}

extern "C" int svc_render_crops_u8(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                                   int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream) {
    const RenderCall c = {"svc_render_crops_u8", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_packed(c, SVC_FMT_RGB24, false);
}
extern "C" int svc_render_crops_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                                     int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream) {
    const RenderCall c = {"svc_render_crops_nv12", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_packed(c, SVC_FMT_NV12, false);
}
extern "C" int svc_render_crops_u8_to_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                                           int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream) {
    const RenderCall c = {"svc_render_crops_u8_to_nv12", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_packed(c, SVC_FMT_RGB24, true);
}
extern "C" int svc_render_crops_nv12_to_nv12(SvcHandle *h, const uint8_t *frames, int n, int height, int width, const int32_t *boxes,
                                             int bw, int bh, uint8_t *out, int oh, int ow, int flags, void *stream) {
    const RenderCall c = {"svc_render_crops_nv12_to_nv12", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_packed(c, SVC_FMT_NV12, true);
}

// --------------------------------------------------------------------------------------
// the same launchers on frames in the caller's layout (SvcFrameLayout: include/svc.h states the rules)
// --------------------------------------------------------------------------------------
// The layout of a height x width picture, checked -> Pitched.  Plain integer comparisons, before any device work.  side: "" for the
// frames' layout, "out_layout: " for an output's (the errors name the side, as colour_check's do; there the picture is the oh x ow
// output and its size rule is the sink's).
static int layout_check(const char *name, const char *side, const SvcFrameLayout *lay, int n, int height, int width, Pitched &L) {
    const bool out = side[0] != 0;
    if (!lay) {
        svc_set_error("%s: %slayout is NULL", name, side);
        return SVC_E_INVALID;
    }
    if (lay->struct_size != sizeof(SvcFrameLayout)) {
        svc_set_error("%s: %sSvcFrameLayout.struct_size is %u, this library's is %zu (a stale binding)", name, side, lay->struct_size,
                      sizeof(SvcFrameLayout));
        return SVC_E_INVALID;
    }
    const bool nv12 = lay->pix_fmt == SVC_FMT_NV12;
    if (!nv12 && lay->pix_fmt != SVC_FMT_RGB24) {
        svc_set_error("%s: %sunknown pix_fmt %d (SVC_FMT_RGB24 or SVC_FMT_NV12)", name, side, lay->pix_fmt);
        return SVC_E_INVALID;
    }
    if (!(nv12 ? SrcNv12<Pitched>::size_ok(height, width) : SrcRgb<Pitched>::size_ok(height, width))) {       // (the sinks' size_ok are these)
        if (out) svc_set_error("%s: %san output of %dx%d (%s)", name, side, width, height, nv12 ? DstNv12<>::size_rule() : DstRgb<false>::size_rule());
        else svc_set_error("%s: invalid argument%s", name, nv12 ? SrcNv12<Pitched>::size_rule() : SrcRgb<Pitched>::size_rule());
        return SVC_E_INVALID;
    }
    L = Pitched{lay->frame_stride, lay->pitch, lay->chroma_offset, lay->chroma_pitch};
    if (L.frame_stride < 0 || L.pitch < 0 || L.chroma_offset < 0 || L.chroma_pitch < 0) {
        svc_set_error("%s: %slayout values must be non-negative", name, side);
        return SVC_E_INVALID;
    }
    const long long row = nv12 ? (long long)width : 3ll * width;
    if (L.pitch < row) {
        svc_set_error("%s: %spitch %lld is below the row's %lld bytes", name, side, L.pitch, row);
        return SVC_E_INVALID;
    }
    if (!nv12 && (L.chroma_offset || L.chroma_pitch)) {
        svc_set_error("%s: %schroma_offset and chroma_pitch must be 0 for rgb24", name, side);
        return SVC_E_INVALID;
    }
    if (nv12 && L.chroma_pitch < width) {
        svc_set_error("%s: %schroma_pitch %lld is below the width %d", name, side, L.chroma_pitch, width);
        return SVC_E_INVALID;
    }
    // (128-bit products: a pitch near 2^63 must fail these comparisons, not wrap past them)
    const __int128 luma_end = (__int128)L.pitch * (height - 1) + width;
    if (nv12 && L.chroma_offset < luma_end) {
        svc_set_error("%s: %schroma_offset %lld is below pitch * (height - 1) + width = %lld: the chroma plane overlaps the last luma row",
                      name, side, L.chroma_offset, (long long)luma_end);
        return SVC_E_INVALID;
    }
    const __int128 extent = nv12 ? (__int128)L.chroma_offset + (__int128)L.chroma_pitch * (height / 2 - 1) + width
                                 : (__int128)L.pitch * (height - 1) + 3ll * width;      // = Src::extent(L, height, width)
    if (L.frame_stride < extent) {
        svc_set_error("%s: %sframe_stride %lld is below the frame's extent of %lld bytes", name, side, L.frame_stride, (long long)extent);
        return SVC_E_INVALID;
    }
    // the launchers form frames + (n - 1) * frame_stride + extent in 64 bits: it must be an address
    if (n > 0 && (__int128)(n - 1) * L.frame_stride + extent > (__int128)PTRDIFF_MAX) {
        svc_set_error("%s: %s%d frames of frame_stride %lld span more than PTRDIFF_MAX bytes", name, side, n, L.frame_stride);
        return SVC_E_INVALID;
    }
    return SVC_OK;
}

// the launchers behind the layout entries: `name` is the entry's own, the colours are checked SvcColours (NULL: BT.601 limited)
static int resize_frames_any(const char *name, SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *colour,
                             int n, int height, int width, uint8_t *out, int sh, int sw, void *stream) {
    Pitched L;
    int rc = layout_check(name, "", layout, n, height, width, L), m, r;
    if (rc) return rc;
    const bool nv12 = layout->pix_fmt == SVC_FMT_NV12;
    if ((rc = colour_check(name, "colour", colour, nv12, m, r))) return rc;
    const Colours C = {COLOUR_DEC[m][r], COLOURS_DEFAULT.enc};
    if (nv12) return resize_frames<SrcNv12<Pitched>>(name, h, frames, L, C, n, height, width, out, sh, sw, stream);
    return resize_frames<SrcRgb<Pitched>>(name, h, frames, L, C, n, height, width, out, sh, sw, stream);
}

// What a layout entry renders with: one of the three launchers (MODE_WINDOWS: the call's `win` holds origins, not boxes), here on
// the pairing of the call's formats, for one output layout policy.  The Lanczos and the sub-pixel kernels exist here only, i.e.
// for the Pitched source policy, 2 sources x 3 sinks per output policy: packed frames arrive as the packed layout's values.
// profiles/pitched_frames.json measured that policy within 4 % of the compile-time packed one on the linear kernels; six more
// instances would buy nothing that has been measured.
enum RenderMode { MODE_LINEAR, MODE_LANCZOS, MODE_WINDOWS };
template <class OLay>
static int render_mode(const RenderCall &c, RenderMode mode, int pix_fmt, bool to_nv12, const Pitched &L, const OLay &O) {
    return render_pair<Pitched, OLay>(pix_fmt, to_nv12, c.flags, [&](auto p) {
        typedef typename decltype(p)::Src Src;
        typedef typename decltype(p)::Dst Dst;
        switch (mode) {
        case MODE_LANCZOS: return render_crops_lanczos<Src, Dst>(c, L, O);
        case MODE_WINDOWS: return render_windows<Src, Dst>(c, L, O);
        default: return render_crops<Src, Dst>(c, L, O);
        }
    });
}

// Behind every layout entry: the checks of the layouts and colours (which fill c.C), then render_mode.
// out_layout (svc_render_crops_to_layout, svc_render_windows_q8; NULL for every other entry, whose output is packed and whose format
// is out_fmt): where the bytes of the oh x ow output frames lie.  The pitched sinks are instantiated here only -- i.e. for the
// Pitched source policy, every kernel, 2 sources x 3 sinks -- and an out_layout that holds the packed values runs the packed sinks.
static int render_crops_any(RenderCall &c, RenderMode mode, const SvcFrameLayout *layout, const SvcColour *in_colour, int out_fmt,
                            const SvcFrameLayout *out_layout, const SvcColour *out_colour) {
    Pitched L, O = {0, 0, 0, 0};
    int rc = layout_check(c.name, "", layout, c.n, c.height, c.width, L), mi, ri, mo, ro;
    if (rc) return rc;
    bool packed_out = true;
    if (out_layout) {
        if ((rc = layout_check(c.name, "out_layout: ", out_layout, c.n, c.oh, c.ow, O))) return rc;
        out_fmt = out_layout->pix_fmt;
        packed_out = out_fmt == SVC_FMT_NV12
            ? O.pitch == c.ow && O.chroma_pitch == c.ow && O.chroma_offset == (long long)c.oh * c.ow &&
                  (size_t)O.frame_stride == DstNv12<>::frame_bytes(c.oh, c.ow)
            : O.pitch == 3ll * c.ow && (size_t)O.frame_stride == DstRgb<false>::frame_bytes(c.oh, c.ow);
    } else if (out_fmt != SVC_FMT_RGB24 && out_fmt != SVC_FMT_NV12) {
        svc_set_error("%s: unknown out_fmt %d (SVC_FMT_RGB24 or SVC_FMT_NV12)", c.name, out_fmt);
        return SVC_E_INVALID;
    }
    const bool to_nv12 = out_fmt == SVC_FMT_NV12;
    if ((rc = colour_check(c.name, "in_colour", in_colour, layout->pix_fmt == SVC_FMT_NV12, mi, ri)) ||
        (rc = colour_check(c.name, "out_colour", out_colour, to_nv12, mo, ro)))
        return rc;
    c.C = {COLOUR_DEC[mi][ri], COLOUR_ENC[mo][ro]};
    return packed_out ? render_mode(c, mode, layout->pix_fmt, to_nv12, L, Packed()) : render_mode(c, mode, layout->pix_fmt, to_nv12, L, O);
}

// The same for the entries that take a filter (SVC_FILTER_*).  linear_name: the name SVC_FILTER_LINEAR reports under
// (svc_render_crops_filter forwards to svc_render_crops_layout: its bytes, its errors).
static int render_crops_filtered(RenderCall &c, const char *linear_name, int filter, const SvcFrameLayout *layout, const SvcColour *in_colour,
                                 int out_fmt, const SvcFrameLayout *out_layout, const SvcColour *out_colour) {
    if (filter == SVC_FILTER_LINEAR) c.name = linear_name;
    else if (filter != SVC_FILTER_LANCZOS) {
        svc_set_error("%s: unknown filter %d (SVC_FILTER_LINEAR or SVC_FILTER_LANCZOS)", c.name, filter);
        return SVC_E_INVALID;
    }
    return render_crops_any(c, filter == SVC_FILTER_LINEAR ? MODE_LINEAR : MODE_LANCZOS, layout, in_colour, out_fmt, out_layout, out_colour);
}

extern "C" int svc_resize_frames_layout(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, int n, int height,
                                        int width, uint8_t *out, int sh, int sw, void *stream) {
    return resize_frames_any("svc_resize_frames_layout", h, frames, layout, nullptr, n, height, width, out, sh, sw, stream);
}
extern "C" int svc_render_crops_layout(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, int n, int height,
                                       int width, const int32_t *boxes, int bw, int bh, uint8_t *out, int out_fmt, int oh, int ow,
                                       int flags, void *stream) {
    RenderCall c = {"svc_render_crops_layout", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_any(c, MODE_LINEAR, layout, nullptr, out_fmt, nullptr, nullptr);
}
// svc_render_crops_layout with a choice of filter (include/svc.h)
extern "C" int svc_render_crops_filter(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, int n, int height, int width,
                                       const int32_t *boxes, int bw, int bh, uint8_t *out, int out_fmt, int oh, int ow,
                                       int filter, int flags, void *stream) {
    RenderCall c = {"svc_render_crops_filter", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_filtered(c, "svc_render_crops_layout", filter, layout, nullptr, out_fmt, nullptr, nullptr);
}

// --------------------------------------------------------------------------------------
// the same with the colour of NV12 frames chosen by the caller, per call, in and out (SvcColour: include/svc.h)
// --------------------------------------------------------------------------------------
extern "C" int svc_resize_frames_colour(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *colour, int n,
                                        int height, int width, uint8_t *out, int sh, int sw, void *stream) {
    return resize_frames_any("svc_resize_frames_colour", h, frames, layout, colour, n, height, width, out, sh, sw, stream);
}
extern "C" int svc_render_crops_colour(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *in_colour, int n,
                                       int height, int width, const int32_t *boxes, int bw, int bh, uint8_t *out, int out_fmt,
                                       const SvcColour *out_colour, int oh, int ow, int filter, int flags, void *stream) {
    RenderCall c = {"svc_render_crops_colour", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return render_crops_filtered(c, c.name, filter, layout, in_colour, out_fmt, nullptr, out_colour);
}

// --------------------------------------------------------------------------------------
// the same into the caller's output layout: an encoder's surfaces (include/svc.h states the write contract)
// --------------------------------------------------------------------------------------
static int out_layout_null(const char *name) {
    svc_set_error("%s: out_layout: layout is NULL", name);
    return SVC_E_INVALID;
}

extern "C" int svc_render_crops_to_layout(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *in_colour,
                                          int n, int height, int width, const int32_t *boxes, int bw, int bh, uint8_t *out,
                                          const SvcFrameLayout *out_layout, const SvcColour *out_colour, int oh, int ow, int filter, int flags,
                                          void *stream) {
    RenderCall c = {"svc_render_crops_to_layout", h, frames, n, height, width, boxes, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return out_layout ? render_crops_filtered(c, c.name, filter, layout, in_colour, 0, out_layout, out_colour) : out_layout_null(c.name);
}

// --------------------------------------------------------------------------------------
// the same at sub-pixel window origins: INTER_LINEAR taps shifted by a per-frame phase (include/svc.h states the arithmetic)
// --------------------------------------------------------------------------------------
extern "C" int svc_render_windows_q8(SvcHandle *h, const uint8_t *frames, const SvcFrameLayout *layout, const SvcColour *in_colour,
                                     int n, int height, int width, const int32_t *origins_q8, int bw, int bh, uint8_t *out,
                                     const SvcFrameLayout *out_layout, const SvcColour *out_colour, int oh, int ow, int flags, void *stream) {
    RenderCall c = {"svc_render_windows_q8", h, frames, n, height, width, origins_q8, bw, bh, out, oh, ow, flags, stream, COLOURS_DEFAULT};
    return out_layout ? render_crops_any(c, MODE_WINDOWS, layout, in_colour, 0, out_layout, out_colour) : out_layout_null(c.name);
}

// --------------------------------------------------------------------------------------
// the five-panel demo frames: a consumer beside the renderer, not inside it (include/svc.h states every rule: svc_demo_frames_u8)
//   k_demo_frames    framex | smaps_orig | smaps | addWeighted | framex side by side, marks on top    smartVidCrop.py:1924-2126
// A workgroup composes DEMO_ROWS output rows of one frame.  Its first wavefront looks at the frame's marks once -- at most
// SVC_DEMO_MAX_MARKS = one lane each --, drops the ignored ones and those whose bounding box misses the workgroup's rows or their
// own panel, and leaves the rest in LDS in list order (ballot + prefix count) with the box in row coordinates; a pixel then walks
// that list with one box test per mark.  Rows are stored like the render kernels': 16-byte groups where the row's address
// allows them, its head and tail bytewise, so that no byte outside out is written whatever its phase (a row is 15 pw bytes).
// --------------------------------------------------------------------------------------
constexpr int DEMO_TB = 256, DEMO_ROWS = 4;
constexpr int DEMO_COORD = 32767, DEMO_SPRITE = 4096;
// a kept mark: its 8 words, then its box in row pixels [panel * pw + x] and rows, inclusive
enum { DM_BX0 = SVC_MARK_WORDS, DM_BX1, DM_BY0, DM_BY1, DM_WORDS };
struct DemoArgs {
    const uint8_t *small, *raw, *filt, *atlas;
    const int32_t *map_of, *marks, *first;
    uint8_t *out;
    long long atlas_bytes;
    int n, ph, pw, n_maps, n_marks, bands, bgr;
};

__device__ __forceinline__ int demo_mean_even(int a, int b) {          // (a + b) / 2, ties to even
    const int s = a + b;
    int v = s >> 1;
    v += s & v & 1;
    return v;
}
__device__ __forceinline__ int demo_blend(int c, int d, int a) { return (c * a + d * (255 - a) + 127) / 255; }

// whether mark M covers pixel (x, y) of its panel (already inside M's box), and with which coverage
__device__ __forceinline__ bool demo_covers(const DemoArgs &A, const int *M, int x, int y, int &a) {
    const int kind = M[0] & 0xff, x0 = M[1], y0 = M[2], x1 = M[3], y1 = M[4], p = M[5];
    a = 255;
    if (kind == SVC_MARK_DISC) {
        const int dx = x - x0, dy = y - y0;                               // (inside the box: |dx|, |dy| <= p <= 255)
        return dx * dx + dy * dy <= p * p;
    }
    if (kind == SVC_MARK_LINE) {
        const long long dx = x1 - x0, dy = y1 - y0, ex = x - x0, ey = y - y0, p2 = (long long)p * p;
        const long long L = dx * dx + dy * dy, u = ex * dx + ey * dy;
        if (L == 0 || u <= 0) return 4 * (ex * ex + ey * ey) <= p2;
        if (u >= L) {
            const long long fx = x - x1, fy = y - y1;
            return 4 * (fx * fx + fy * fy) <= p2;
        }
        const long long c = ex * dy - ey * dx, ac = c < 0 ? -c : c;
        return ac < (1ll << 31) && ac * ac <= ((p2 * L) >> 2);           // 4 c^2 <= p^2 L, p^2 L < 2^50
    }
    if (kind == SVC_MARK_RECT) return x == x0 || x == x1 || y == y0 || y == y1;
    const long long at = (long long)p + (long long)(y - y0) * (M[6] & 0xffff) + (x - x0);      // SVC_MARK_TEXT
    if (at < 0 || at >= A.atlas_bytes) return false;
    a = A.atlas[at];
    return true;
}

// pixel px (0 .. 5 pw - 1) of row y of frame f, marks applied -> c0 | c1 << 8 | c2 << 16 in output channel order
__device__ __forceinline__ uint32_t demo_pixel(const DemoArgs &A, const int (*marks)[DM_WORDS], int n_kept, int f, long long m, int y, int px) {
    const int pw = A.pw;
    const int k = (px >= pw) + (px >= 2 * pw) + (px >= 3 * pw) + (px >= 4 * pw), x = px - k * pw;
    int r, g, b;
    if (k == 1 || k == 2) {
        r = g = b = m >= 0 ? (k == 1 ? A.raw : A.filt)[((size_t)m * A.ph + y) * pw + x] : 0;
    } else {
        const uint8_t *S = A.small + (((size_t)f * A.ph + y) * pw + x) * 3;
        r = S[0], g = S[1], b = S[2];
        if (k == 3) {
            const int v = m >= 0 ? A.filt[((size_t)m * A.ph + y) * pw + x] : 0;
            r = demo_mean_even(r, v), g = demo_mean_even(g, v), b = demo_mean_even(b, v);
        }
    }
    for (int i = 0; i < n_kept; ++i) {
        const int *M = marks[i];                                          // (a uniform address: one LDS broadcast)
        if (px < M[DM_BX0] || px > M[DM_BX1] || y < M[DM_BY0] || y > M[DM_BY1]) continue;
        int a;
        if (!demo_covers(A, M, x, y, a)) continue;
        const int col = M[7];
        r = demo_blend(col & 255, r, a), g = demo_blend((col >> 8) & 255, g, a), b = demo_blend((col >> 16) & 255, b, a);
    }
    return A.bgr ? (uint32_t)b | (uint32_t)g << 8 | (uint32_t)r << 16 : (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16;
}

__global__ __launch_bounds__(DEMO_TB) void k_demo_frames(DemoArgs A) {
    __shared__ int s_marks[SVC_DEMO_MAX_MARKS][DM_WORDS];
    __shared__ int s_kept;
    const int tid = threadIdx.x, f = (int)blockIdx.x / A.bands, band = (int)blockIdx.x - f * A.bands;
    const int yb0 = band * DEMO_ROWS, yb1 = min(A.ph, yb0 + DEMO_ROWS) - 1;
    if (tid < 64) {                                                       // the first wavefront, whole: one lane per mark
        const int lo = min(max(A.first[f], 0), A.n_marks), hi = min(max(A.first[f + 1], 0), A.n_marks);
        const int cnt = min(max(hi - lo, 0), SVC_DEMO_MAX_MARKS);
        int w[DM_WORDS];
        bool keep = false;
        if (tid < cnt) {
            const int32_t *mp = A.marks + (size_t)(lo + tid) * SVC_MARK_WORDS;
#pragma unroll
            for (int i = 0; i < SVC_MARK_WORDS; ++i) w[i] = mp[i];
            const int kind = w[0] & 0xff, panel = w[0] >> 8, p = w[5], q = w[6];
            bool ok = w[0] >= 0 && kind <= SVC_MARK_TEXT && panel < SVC_DEMO_PANELS;
#pragma unroll
            for (int i = 1; i <= 4; ++i) ok = ok && w[i] >= -DEMO_COORD && w[i] <= DEMO_COORD;
            int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
            if (ok) {
                if (kind == SVC_MARK_DISC || kind == SVC_MARK_LINE) {
                    ok = p >= 0 && p <= 255;
                    const int rad = kind == SVC_MARK_DISC ? p : (p + 1) >> 1;
                    const int ex = kind == SVC_MARK_DISC ? w[1] : w[3], ey = kind == SVC_MARK_DISC ? w[2] : w[4];
                    bx0 = min(w[1], ex) - rad, bx1 = max(w[1], ex) + rad, by0 = min(w[2], ey) - rad, by1 = max(w[2], ey) + rad;
                } else if (kind == SVC_MARK_RECT) {
                    bx0 = w[1], bx1 = w[3], by0 = w[2], by1 = w[4];
                } else {
                    const int sw = q & 0xffff, sh = q >> 16;
                    ok = q >= 0 && sw <= DEMO_SPRITE && sh <= DEMO_SPRITE;
                    bx0 = w[1], bx1 = w[1] + sw - 1, by0 = w[2], by1 = w[2] + sh - 1;
                }
            }
            bx0 = max(bx0, 0), bx1 = min(bx1, A.pw - 1), by0 = max(by0, yb0), by1 = min(by1, yb1);       // its own panel, this workgroup's rows
            keep = ok && bx0 <= bx1 && by0 <= by1;
            w[DM_BX0] = panel * A.pw + bx0, w[DM_BX1] = panel * A.pw + bx1, w[DM_BY0] = by0, w[DM_BY1] = by1;
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const int slot = __popcll(mask & ((1ull << tid) - 1ull));
#pragma unroll
            for (int i = 0; i < DM_WORDS; ++i) s_marks[slot][i] = w[i];
        }
        if (tid == 0) s_kept = __popcll(mask);
    }
    __syncthreads();
    const int n_kept = s_kept;
    const long long mm = A.map_of[f], m = mm >= 0 && mm < A.n_maps ? mm : -1;
    const int rowb = 15 * A.pw;
    for (int y = yb0; y <= yb1; ++y) {
        uint8_t *row = A.out + ((size_t)f * A.ph + y) * (size_t)rowb;
        const int head = min(rowb, (int)((16 - ((uintptr_t)row & 15)) & 15)), nvec = (rowb - head) >> 4, tail = rowb - head - 16 * nvec;
        for (int i = tid; i < nvec + 2; i += DEMO_TB) {                  // item 0: the head; 1 .. nvec: the 16-byte groups; nvec + 1: the tail
            const int b0 = i == 0 ? 0 : head + 16 * (min(i, nvec + 1) - 1), cnt = i == 0 ? head : i <= nvec ? 16 : tail;
            if (cnt == 0) continue;
            uint64_t lo = 0, hi = 0;                                      // bytes b0 .. b0 + 15 of the row
            const int p0 = b0 / 3, p1 = (b0 + cnt - 1) / 3;
            for (int p = p0; p <= p1; ++p) {
                const uint32_t v = demo_pixel(A, s_marks, n_kept, f, m, y, p);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int q = 3 * p + c - b0;
                    const uint64_t byte = (v >> (8 * c)) & 255u;
                    if (q >= 0 && q < 8) lo |= byte << (8 * q);
                    else if (q >= 8 && q < 16) hi |= byte << (8 * (q - 8));
                }
            }
            if (cnt == 16) {
                *(uint4 *)(row + b0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
            } else {
                for (int q = 0; q < cnt; ++q) row[b0 + q] = (uint8_t)(q < 8 ? lo >> (8 * q) : hi >> (8 * (q - 8)));
            }
        }
    }
}

// No handle: no weights, no scratch, no state -- callable from any thread on any stream of the current device.
extern "C" int svc_demo_frames_u8(const uint8_t *small, int n, int ph, int pw, const uint8_t *raw, const uint8_t *filt, int n_maps,
                                  const int32_t *map_of, const int32_t *marks, int n_marks, const int32_t *first,
                                  const uint8_t *atlas, size_t atlas_bytes, uint8_t *out, int flags, void *stream) {
    const char *rule = nullptr;
    if (n < 0 || n_maps < 0 || n_marks < 0) rule = "a count (n, n_maps, n_marks) is negative";
    else if (ph < 1 || pw < 1) rule = "ph or pw is below 1";
    else if (pw > 0x7fffffff / 15) rule = "a row of 15 pw bytes is beyond 2^31 - 1";
    else if (flags & ~SVC_RENDER_BGR) rule = "flags has bits other than SVC_RENDER_BGR";
    else if (n > 0 && (!small || !map_of || !first || !out)) rule = "small, map_of, first or out is NULL with n > 0";
    else if (n > 0 && n_maps > 0 && (!raw || !filt)) rule = "raw or filt is NULL with n_maps > 0";
    else if (n > 0 && n_marks > 0 && !marks) rule = "marks is NULL with n_marks > 0";
    else if (n > 0 && atlas_bytes > 0 && !atlas) rule = "atlas is NULL with atlas_bytes > 0";
    const int bands = rule ? 0 : (ph - 1) / DEMO_ROWS + 1;
    if (!rule && (long long)n * bands > 0x7fffffffll) rule = "n * ceil(ph / 4) workgroups are beyond 2^31 - 1";
    if (rule) {
        svc_set_error("svc_demo_frames_u8: %s (n %d, ph %d, pw %d, n_maps %d, n_marks %d, flags %d)", rule, n, ph, pw, n_maps, n_marks, flags);
        return SVC_E_INVALID;
    }
    if (n == 0) return SVC_OK;
    const long long ab = atlas_bytes > (size_t)0x7fffffffffffffffll ? 0x7fffffffffffffffll : (long long)atlas_bytes;
    const DemoArgs A = {small, raw, filt, atlas, map_of, marks, first, out, ab, n, ph, pw, n_maps, n_marks, bands, flags & SVC_RENDER_BGR};
    k_demo_frames<<<(unsigned)(n * bands), DEMO_TB, 0, (hipStream_t)stream>>>(A);
    SVC_CHECK_LAUNCH();
    return SVC_OK;
}
