// segm.hip — COCO polygon and RLE segmentations rasterised on the device (datasets/segm.py): annToMask without pycocotools.
//
// The rule is maskApi.c's rleFrPoly / rleMerge (union) / rleDecode.  A polygon part is walked on a 5x grid; wherever two consecutive
// points of an edge differ in u and the column between them is a pixel column of the image, the outline TOGGLES the column-major
// flat index xd * h + yd, and cell i is ON iff the number of toggles a <= i is odd.  An RLE is its toggle list already (the cumulative
// sums of its run lengths).  The library sorts the toggles and merges zero-length runs; the parity below is the same thing.
//
// Toggle launches: one lane per (edge, step).  A lane finds its edge in the prefix table of step counts by bisection and evaluates
// the two points of its pair from the closed formulas (float64, one rounding per operation in the library's order: this file is
// built with -ffp-contract=off), so there is no sequential walk.  It flips ONE bit of its part's toggle bitmap with atomicXor: XOR
// is order-independent and two toggles at one index cancel, as the rule requires, so the bytes are the same on every run.  The RLE
// launch flips the bits of the uploaded lists the same way.
//
// Bitmap of a part (workspace, zeroed by the entry point): the columns of its instance's rectangle, h + 1 slots each (yd = h, "the
// first cell of the next column", is slot h: it counts for every later column and for no cell of its own), 64 slots per word, word k
// of column c at [k * rw + c] so that lanes on consecutive columns read consecutive words.
//
// Fill launch: workgroup = 64 columns x 512 rows of one instance's rectangle.  Each of the four waves takes every fourth part: per
// column the parity of everything before the tile's first row (earlier columns, then earlier words of the column) is a popcount
// fold; inside a word the prefix parity is six shift-XORs.  Parts are ORed in registers, the four waves' words meet in LDS (the
// column-major to row-major turn), and the stores run along rows: 64 consecutive bytes per wave.  Ordinary stores only.
//
// mpn_segm_mask_miss shares the toggle launches and the per-part words (or_part_words) and replaces the fill launch by a compose
// launch per IMAGE tile: the image's person annotations are walked in order and combined by kind into mask_miss, without any
// instance mask in memory (segm_mask_miss_kernel).
#include "common.h"

namespace {

constexpr int SEG_KC = 8;                        // words (of 64 rows) per fill tile
constexpr int SEG_MAX_ABS = 5 * (1 << 20) + 1;   // |X|, |Y| of an upsampled vertex the packer can produce

struct SegInst {
    int h, w, rx0, ry0, rw, rh, p0, p1;
    long off, pitch;
    bool ok;
};

// Instance row -> registers.  `ok` guards every use: a row whose rectangle leaves the image, whose parts leave the part table or
// whose output leaves the buffer is skipped, never dereferenced (the host wrapper never produces one).  out_bytes < 0: the OUT
// columns are not used by this launch (mask_miss writes whole image planes) and are not looked at.
__device__ __forceinline__ SegInst load_inst(const int64_t* __restrict__ row, int n_parts, long out_bytes) {
    SegInst s;
    const int64_t h = row[MPN_SEGI_H], w = row[MPN_SEGI_W], x0 = row[MPN_SEGI_RX0], y0 = row[MPN_SEGI_RY0], rw = row[MPN_SEGI_RW],
                  rh = row[MPN_SEGI_RH], p0 = row[MPN_SEGI_P0], p1 = row[MPN_SEGI_P1];
    s.off = row[MPN_SEGI_OUT_OFF];
    s.pitch = row[MPN_SEGI_OUT_PITCH];
    s.ok = h >= 1 && h <= 65536 && w >= 1 && w <= 65536 && h * w <= 0x7fffffffL && x0 >= 0 && y0 >= 0 && rw >= 1 && rh >= 1 &&
           x0 <= w - rw && y0 <= h - rh && p0 >= 0 && p0 <= p1 && p1 <= n_parts;
    if (out_bytes >= 0)
        s.ok = s.ok && s.off >= 0 && s.pitch >= rw && s.off <= out_bytes && s.pitch <= out_bytes && (rh - 1) * s.pitch + rw <= out_bytes - s.off;
    s.h = s.ok ? (int)h : 1; s.w = s.ok ? (int)w : 1;
    s.rx0 = s.ok ? (int)x0 : 0; s.ry0 = s.ok ? (int)y0 : 0; s.rw = s.ok ? (int)rw : 1; s.rh = s.ok ? (int)rh : 1;
    s.p0 = s.ok ? (int)p0 : 0; s.p1 = s.ok ? (int)p1 : 0;
    return s;
}

struct SegPart {
    SegInst in;
    int v0, v1;
    unsigned long long* bm;
    bool ok;
};

// Part row -> registers, with its instance.  ok: the part belongs to an instance that lists it and its bitmap lies in the workspace.
__device__ __forceinline__ SegPart load_part(int p, const int64_t* __restrict__ parts, int n_parts, const int64_t* __restrict__ insts,
                                             int n_inst, int n_verts, long out_bytes, unsigned long long* ws, long ws_words) {
    SegPart s;
    s.ok = false;
    s.bm = ws;
    s.v0 = s.v1 = 0;
    s.in.ok = false;
    if (p < 0 || p >= n_parts) return s;
    const int64_t* row = parts + (long)p * MPN_SEGP_COLS;
    const int64_t inst = row[MPN_SEGP_INST], v0 = row[MPN_SEGP_V0], v1 = row[MPN_SEGP_V1], bm = row[MPN_SEGP_BM];
    if (inst < 0 || inst >= n_inst) return s;
    s.in = load_inst(insts + inst * MPN_SEGI_COLS, n_parts, out_bytes);
    if (!s.in.ok || p < s.in.p0 || p >= s.in.p1) return s;
    const long words = (long)(s.in.h / 64 + 1) * s.in.rw;
    if (v0 < 0 || v0 > v1 || v1 > n_verts || bm < 0 || bm > ws_words || words > ws_words - bm) return s;
    s.v0 = (int)v0; s.v1 = (int)v1;
    s.bm = ws + bm;
    s.ok = true;
    return s;
}

// the toggle (column xd, slot yd in 0 .. h): columns outside the instance's rectangle hold no ON cell and have no slot
__device__ __forceinline__ void flip_bit(const SegPart& pt, int xd, int yd) {
    const int c = xd - pt.in.rx0;
    if (c < 0 || c >= pt.in.rw || yd < 0 || yd > pt.in.h) return;
    atomicXor(pt.bm + (long)(yd >> 6) * pt.in.rw + c, 1ull << (yd & 63));
}

__global__ void __launch_bounds__(256) segm_toggle_poly_kernel(const int32_t* __restrict__ verts, const int32_t* __restrict__ vpart,
                                                               const int32_t* __restrict__ estart, int n_verts, long n_steps,
                                                               const int64_t* __restrict__ parts, int n_parts,
                                                               const int64_t* __restrict__ insts, int n_inst, long out_bytes,
                                                               unsigned long long* ws, long ws_words) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_steps) return;
    // the edge of this step: the last e with estart[e] <= g (edges without a step share their successor's entry and are never found)
    int lo = 0, hi = n_verts;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)estart[mid] <= g) lo = mid; else hi = mid;
    }
    const int e = lo;
    const long i = g - (long)estart[e];
    const SegPart pt = load_part(vpart[e], parts, n_parts, insts, n_inst, n_verts, out_bytes, ws, ws_words);
    if (!pt.ok || e < pt.v0 || e >= pt.v1 || i < 0) return;
    const int q = e + 1 == pt.v1 ? pt.v0 : e + 1;
    int xs = verts[2 * e], ys = verts[2 * e + 1], xe = verts[2 * q], ye = verts[2 * q + 1];
    if (abs(xs) > SEG_MAX_ABS || abs(ys) > SEG_MAX_ABS || abs(xe) > SEG_MAX_ABS || abs(ye) > SEG_MAX_ABS) return;
    const int dx = abs(xe - xs), dy = abs(ys - ye), n = max(dx, dy);
    if (i >= n) return;                                              // a table whose step counts are not the vertices'
    const bool flat = dx >= dy;
    const bool flip = (flat && xs > xe) || (!flat && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    const double s = flat ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
    // points d = i and d = i + 1 of the walk from P to Q
    int u[2], v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int d = (int)i + k, t = flip ? n - d : d;
        if (flat) { u[k] = t + xs; v[k] = (int)(ys + s * t + .5); }
        else      { v[k] = t + ys; u[k] = (int)(xs + s * t + .5); }
    }
    if (u[1] == u[0]) return;
    double xd = (double)(u[1] < u[0] ? u[1] : u[1] - 1);
    xd = (xd + .5) / 5.0 - .5;
    if (floor(xd) != xd || xd < 0 || xd > pt.in.w - 1) return;
    double yd = (double)(v[1] < v[0] ? v[1] : v[0]);
    yd = (yd + .5) / 5.0 - .5;
    if (yd < 0) yd = 0; else if (yd > pt.in.h) yd = pt.in.h;
    yd = ceil(yd);
    flip_bit(pt, (int)xd, (int)yd);
}

__global__ void __launch_bounds__(256) segm_toggle_rle_kernel(const int32_t* __restrict__ toggles, int n_tog,
                                                              const int64_t* __restrict__ parts, int n_parts,
                                                              const int64_t* __restrict__ insts, int n_inst, int n_verts, long out_bytes,
                                                              unsigned long long* ws, long ws_words) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= n_tog) return;
    const int a = toggles[2 * g + 1];
    const SegPart pt = load_part(toggles[2 * g], parts, n_parts, insts, n_inst, n_verts, out_bytes, ws, ws_words);
    if (!pt.ok || a < 0 || (long)a >= (long)pt.in.h * pt.in.w) return;      // a = h * w has no effect
    flip_bit(pt, a / pt.in.h, a % pt.in.h);
}

__device__ __forceinline__ unsigned long long wave_parity(unsigned long long bit) { return __popcll(__ballot((bit & 1) != 0)) & 1; }

// The words k0 .. k0 + NW - 1 (64 rows each) of ONE part at rectangle column c, ORed into acc: bit b of word k = the cell is ON.
// bm: the part's bitmap (rw columns, cw words each).  c0: the rectangle column of the wave's lane 0 (c = c0 + lane; it may be
// negative, and lanes with cin false lie outside the rectangle and get nothing).  Per column the parity of everything before
// word k0 (earlier columns, then earlier words of the column) is a popcount fold; inside a word the prefix parity is six
// shift-XORs.  Every lane of the wave must call this together (ballots).
template <int NW>
__device__ __forceinline__ void or_part_words(const unsigned long long* __restrict__ bm, int rw, int cw, int c0, int c, bool cin, int k0,
                                              int lane, unsigned long long (&acc)[NW]) {
    // parity of every toggle in the columns before this tile (an RLE run may span columns; a closed outline leaves none)
    unsigned long long base = 0;
    for (int cc = lane; cc < c0; cc += 64)
        for (int k = 0; k < cw; ++k) base ^= (unsigned long long)__popcll(bm[(long)k * rw + cc]);
    base = wave_parity(base);
    // this column: all of it (for the columns to its right) and what lies above the tile
    unsigned long long tot = 0, pre = 0;
    if (cin)
        for (int k = 0; k < cw; ++k) {
            const unsigned long long pc = (unsigned long long)__popcll(bm[(long)k * rw + c]) & 1;
            tot ^= pc;
            if (k < k0) pre ^= pc;
        }
    const unsigned long long left = __popcll(__ballot(tot != 0) & ((1ull << lane) - 1)) & 1;
    unsigned long long run = base ^ left ^ pre;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int k = k0 + j;
        if (cin && k < cw) {
            const unsigned long long wd = bm[(long)k * rw + c];
            unsigned long long y = wd;                             // bit i = parity of bits 0 .. i
            y ^= y << 1; y ^= y << 2; y ^= y << 4; y ^= y << 8; y ^= y << 16; y ^= y << 32;
            acc[j] |= run ? ~y : y;
            run ^= (unsigned long long)__popcll(wd) & 1;
        }
    }
}

// Bitmap of part p of instance `inst` (p lies inside the part table: load_inst), or null: the part must name this instance and its
// bitmap must lie in the workspace.
__device__ __forceinline__ const unsigned long long* part_bitmap(const int64_t* __restrict__ parts, int p, int inst, const SegInst& in,
                                                                 const unsigned long long* __restrict__ ws, long ws_words) {
    const int64_t off = parts[(long)p * MPN_SEGP_COLS + MPN_SEGP_BM];
    if (parts[(long)p * MPN_SEGP_COLS + MPN_SEGP_INST] != inst || off < 0 || off > ws_words || (long)(in.h / 64 + 1) * in.rw > ws_words - off)
        return nullptr;
    return ws + off;
}

__global__ void __launch_bounds__(256) segm_fill_kernel(const int64_t* __restrict__ parts, int n_parts, const int64_t* __restrict__ insts,
                                                        const unsigned long long* __restrict__ ws, long ws_words,
                                                        uint8_t* __restrict__ out, long out_bytes, int32_t* __restrict__ any_on) {
    __shared__ unsigned long long slab[4][SEG_KC][64];
    const int inst = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SegInst in = load_inst(insts + (long)inst * MPN_SEGI_COLS, n_parts, out_bytes);
    const int c0 = blockIdx.x * 64;
    const int cw = in.h / 64 + 1, k_last = (in.ry0 + in.rh - 1) >> 6, k0 = (in.ry0 >> 6) + blockIdx.y * SEG_KC;
    if (!in.ok || c0 >= in.rw || k0 > k_last) return;                 // the same for the whole workgroup
    const int c = c0 + lane;
    const bool cin = c < in.rw;
    unsigned long long acc[SEG_KC];
#pragma unroll
    for (int j = 0; j < SEG_KC; ++j) acc[j] = 0;
    for (int p = in.p0 + wave; p < in.p1; p += 4) {
        const unsigned long long* bm = part_bitmap(parts, p, inst, in, ws, ws_words);
        if (bm) or_part_words<SEG_KC>(bm, in.rw, cw, c0, c, cin, k0, lane, acc);          // the same for the whole wave
    }
#pragma unroll
    for (int j = 0; j < SEG_KC; ++j) slab[wave][j][lane] = acc[j];
    __syncthreads();
    // rows: wave `wave` stores rows wave, wave + 4, ... of every word; a wave's 64 lanes are 64 consecutive bytes of one row
    bool on = false;
#pragma unroll 1
    for (int j = 0; j < SEG_KC; ++j) {
        const int k = k0 + j;
        if (k > k_last) break;
        const unsigned long long wd = slab[0][j][lane] | slab[1][j][lane] | slab[2][j][lane] | slab[3][j][lane];
        for (int b = wave; b < 64; b += 4) {
            const int r = k * 64 + b - in.ry0;
            if (cin && r >= 0 && r < in.rh) {
                const uint8_t bit = (uint8_t)((wd >> b) & 1);
                out[in.off + (long)r * in.pitch + c] = bit;
                on = on || bit != 0;
            }
        }
    }
    // zeroed by the entry point; every writer stores the same 1
    if (__ballot(on) != 0 && lane == 0) any_on[inst] = 1;
}

struct SegImg {
    int h, w, i0, i1;
    long off, pitch;
    bool ok;
};

// Image row -> registers.  ok: its instances lie in the instance table and its H x W plane lies in the output.
__device__ __forceinline__ SegImg load_img(const int64_t* __restrict__ row, int n_inst, long out_bytes) {
    SegImg s;
    const int64_t h = row[MPN_SEGM_H], w = row[MPN_SEGM_W], i0 = row[MPN_SEGM_I0], i1 = row[MPN_SEGM_I1];
    s.off = row[MPN_SEGM_OUT_OFF];
    s.pitch = row[MPN_SEGM_OUT_PITCH];
    s.ok = h >= 1 && h <= 65536 && w >= 1 && w <= 65536 && h * w <= 0x7fffffffL && i0 >= 0 && i0 <= i1 && i1 <= n_inst;
    s.ok = s.ok && s.off >= 0 && s.pitch >= w && s.off <= out_bytes && s.pitch <= out_bytes && (h - 1) * s.pitch + w <= out_bytes - s.off;
    s.h = s.ok ? (int)h : 1; s.w = s.ok ? (int)w : 1;
    s.i0 = s.ok ? (int)i0 : 0; s.i1 = s.ok ? (int)i1 : 0;
    return s;
}

// bits lo .. hi - 1 of a word (any lo, hi; empty when hi <= lo)
__device__ __forceinline__ unsigned long long bit_range(int lo, int hi) {
    if (hi <= 0 || lo >= 64 || hi <= lo) return 0;
    const unsigned long long below_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1;
    return lo <= 0 ? below_hi : below_hi & (~0ull << lo);
}

// mask_miss of one image from its person annotations IN ORDER (datasets/segm.py states the rule): workgroup = 64 image columns x
// 512 image rows of one image.  Wave v owns words 2 v and 2 v + 1 of the tile's eight through every instance, so `all` and `miss`
// stay in its registers and nothing crosses waves before the turn: for an instance whose rectangle meets its words it ORs the
// instance's parts (or_part_words, image column x = rectangle column x - rx0, cells outside the rectangle read 0) and only then
// applies the kind.  ~miss goes column-major -> row-major through LDS (4 KiB) and is stored as 0 / 255 along rows, four bytes per lane
// where the plane's rows are 4-byte aligned.  No atomics: the bytes are the same on every run.
//
// ALL (mpn_segm_person_masks): the same walk also keeps `uni`, the union of EVERY instance whatever its kind (all | crowds), and stores
// it as a second plane, mask_all, at the same offset and pitch of out_all: 255 where anyone stands.  With ALL false `uni`, its slab
// and its stores do not exist and the kernel is mpn_segm_mask_miss's as it always was.
template <bool ALL>
__global__ void __launch_bounds__(256) segm_mask_miss_kernel(const int64_t* __restrict__ imgs, const int64_t* __restrict__ insts, int n_inst,
                                                             const int32_t* __restrict__ kind, const int64_t* __restrict__ parts, int n_parts,
                                                             const unsigned long long* __restrict__ ws, long ws_words,
                                                             uint8_t* __restrict__ out, uint8_t* __restrict__ out_all, long out_bytes) {
    constexpr int NW = SEG_KC / 4;                                       // words per wave
    __shared__ unsigned long long slab[ALL ? 2 : 1][SEG_KC][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SegImg im = load_img(imgs + (long)blockIdx.z * MPN_SEGM_COLS, n_inst, out_bytes);
    const int x0 = blockIdx.x * 64, k0 = blockIdx.y * SEG_KC;
    if (!im.ok || x0 >= im.w || k0 * 64 >= im.h) return;                 // the same for the whole workgroup
    const int kw = k0 + wave * NW;                                       // this wave's first word
    unsigned long long all[NW], miss[NW], uni[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) all[j] = miss[j] = uni[j] = 0;
    for (int i = im.i0; i < im.i1; ++i) {
        const SegInst in = load_inst(insts + (long)i * MPN_SEGI_COLS, n_parts, -1);
        const int kd = kind[i];
        if (!in.ok || in.h != im.h || in.w != im.w || kd < MPN_SEGK_KEYPOINTS || kd > MPN_SEGK_CROWD) continue;
        // the rectangle misses the tile: the same for the whole workgroup
        if (in.rx0 >= x0 + 64 || in.rx0 + in.rw <= x0 || in.ry0 >= (k0 + SEG_KC) * 64 || in.ry0 + in.rh <= k0 * 64) continue;
        // ... or this wave's words of it: the same for the whole wave
        if (in.ry0 >= (kw + NW) * 64 || in.ry0 + in.rh <= kw * 64) continue;
        const int c = x0 + lane - in.rx0, cw = in.h / 64 + 1;
        const bool cin = c >= 0 && c < in.rw;
        unsigned long long m[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) m[j] = 0;
        for (int p = in.p0; p < in.p1; ++p) {
            const unsigned long long* bm = part_bitmap(parts, p, i, in, ws, ws_words);
            if (bm) or_part_words<NW>(bm, in.rw, cw, x0 - in.rx0, c, cin, kw, lane, m);
        }
        // every part is in: now the kind
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const unsigned long long mj = m[j] & bit_range(in.ry0 - (kw + j) * 64, in.ry0 + in.rh - (kw + j) * 64);
            if (ALL) uni[j] |= mj;
            if (kd == MPN_SEGK_CROWD) {
                miss[j] |= mj & ~all[j];
            } else {
                all[j] |= mj;
                if (kd == MPN_SEGK_NO_KEYPOINTS) miss[j] |= mj;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        slab[0][wave * NW + j][lane] = ~miss[j];
        if (ALL) slab[ALL ? 1 : 0][wave * NW + j][lane] = uni[j];
    }
    __syncthreads();
    // rows: a lane holds four consecutive columns, 16 lanes are the 64 bytes of one row, a wave stores four rows at a time; wave v
    // stores rows 16 v .. 16 v + 15 of every word
    const int cg = (lane & 15) * 4, x = x0 + cg;
#pragma unroll
    for (int pl = 0; pl < (ALL ? 2 : 1); ++pl) {
        uint8_t* plane = (pl == 0 ? out : out_all) + im.off;
        const bool wide = (((uintptr_t)plane | (uintptr_t)im.pitch) & 3) == 0 && x + 3 < im.w;
#pragma unroll 1
        for (int j = 0; j < SEG_KC; ++j) {
            if ((k0 + j) * 64 >= im.h) break;
            unsigned long long wd[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) wd[t] = slab[pl][j][cg + t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = wave * 16 + r * 4 + (lane >> 4), y = (k0 + j) * 64 + b;
                if (y >= im.h || x >= im.w) continue;
                uint32_t v = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) v |= (0u - (uint32_t)((wd[t] >> b) & 1) & 0xffu) << (8 * t);
                uint8_t* q = plane + (long)y * im.pitch + x;
                if (wide) {
                    *reinterpret_cast<uint32_t*>(q) = v;
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (x + t < im.w) q[t] = (uint8_t)(v >> (8 * t));
                }
            }
        }
    }
}

// The toggle stage both entry points start with: the workspace zeroed, then one bit flipped per crossing of a polygon outline and
// per listed RLE toggle.  out_bytes < 0: the instances' OUT columns are not checked (load_inst).  Validates what it uses before its
// first HIP call.
int segm_toggle_stage(const int64_t* insts, int n_inst, const int64_t* parts, int n_parts, const int32_t* verts, const int32_t* vpart,
                      const int32_t* estart, int n_verts, int64_t n_steps, const int32_t* toggles, int n_tog, long out_bytes,
                      void* workspace, int64_t ws_bytes, hipStream_t st) {
    MPN_CHECK_ARG(workspace && estart && n_inst >= 0 && n_inst <= 65535 && n_parts >= 0 && n_verts >= 0 && n_tog >= 0 && n_steps >= 0 && n_steps <= 0x7fffffffL);
    MPN_CHECK_ARG((n_inst == 0 || insts) && (n_parts == 0 || parts));
    MPN_CHECK_ARG(n_verts == 0 || (verts && vpart));
    MPN_CHECK_ARG(n_verts > 0 || n_steps == 0);
    MPN_CHECK_ARG(n_tog == 0 || toggles);
    MPN_CHECK_ARG(ws_bytes >= 8 && ws_bytes % 8 == 0 && ws_bytes / 8 <= 0x7fffffffL);
    MPN_CHECK_ARG(((uintptr_t)insts | (uintptr_t)parts | (uintptr_t)workspace) % 8 == 0);
    MPN_CHECK_ARG(((uintptr_t)verts | (uintptr_t)vpart | (uintptr_t)estart | (uintptr_t)toggles) % 4 == 0);
    const long ws_words = (long)(ws_bytes / 8);
    unsigned long long* ws = (unsigned long long*)workspace;
    if (hipMemsetAsync(workspace, 0, (size_t)ws_bytes, st) != hipSuccess) return mpn_launch_status();
    if (n_steps > 0)
        hipLaunchKernelGGL(segm_toggle_poly_kernel, dim3((unsigned)((n_steps + 255) / 256)), dim3(256), 0, st, verts, vpart, estart, n_verts,
                           (long)n_steps, parts, n_parts, insts, n_inst, out_bytes, ws, ws_words);
    if (n_tog > 0)
        hipLaunchKernelGGL(segm_toggle_rle_kernel, dim3((unsigned)((n_tog + 255) / 256)), dim3(256), 0, st, toggles, n_tog, parts, n_parts,
                           insts, n_inst, n_verts, out_bytes, ws, ws_words);
    return mpn_launch_status();
}

}  // namespace

extern "C" int64_t mpn_segm_workspace_bytes(int64_t words) {
    if (words < 0 || words > 0x7fffffffL) return 0;
    return (words > 0 ? words : 1) * 8;
}

extern "C" int mpn_segm_rasterize(const int64_t* insts, int n_inst, const int64_t* parts, int n_parts, const int32_t* verts,
                                  const int32_t* vpart, const int32_t* estart, int n_verts, int64_t n_steps, const int32_t* toggles,
                                  int n_tog, int max_rw, int max_h, uint8_t* out, int64_t out_bytes, int dense, int32_t* any_on,
                                  void* workspace, int64_t ws_bytes, void* stream) {
    MPN_CHECK_ARG(insts && parts && out && any_on && n_inst >= 1);
    MPN_CHECK_ARG(max_rw >= 1 && max_rw <= 65536 && max_h >= 1 && max_h <= 65536 && out_bytes >= 1 && out_bytes <= (1L << 40) && (dense == 0 || dense == 1));
    MPN_CHECK_ARG((uintptr_t)any_on % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    const int rc = segm_toggle_stage(insts, n_inst, parts, n_parts, verts, vpart, estart, n_verts, n_steps, toggles, n_tog, (long)out_bytes,
                                     workspace, ws_bytes, st);
    if (rc != 0) return rc;
    if (hipMemsetAsync(any_on, 0, (size_t)n_inst * sizeof(int32_t), st) != hipSuccess) return mpn_launch_status();
    // dense: the planes are zero outside the rectangles; packed: the rectangles are written whole (the padding between them is not read)
    if (dense && hipMemsetAsync(out, 0, (size_t)out_bytes, st) != hipSuccess) return mpn_launch_status();
    const int words = max_h / 64 + 1;
    dim3 grid((unsigned)((max_rw + 63) / 64), (unsigned)((words + SEG_KC - 1) / SEG_KC), (unsigned)n_inst);
    hipLaunchKernelGGL(segm_fill_kernel, grid, dim3(256), 0, st, parts, n_parts, insts, (const unsigned long long*)workspace, (long)(ws_bytes / 8),
                       out, (long)out_bytes, any_on);
    return mpn_launch_status();
}

// what mpn_segm_mask_miss and mpn_segm_person_masks share: out_all null = the one-plane form
static int segm_compose(const int64_t* imgs, int n_img, const int64_t* insts, const int32_t* kind, int n_inst, const int64_t* parts,
                        int n_parts, const int32_t* verts, const int32_t* vpart, const int32_t* estart, int n_verts, int64_t n_steps,
                        const int32_t* toggles, int n_tog, int max_w, int max_h, uint8_t* out, uint8_t* out_all, int64_t out_bytes,
                        void* workspace, int64_t ws_bytes, void* stream) {
    MPN_CHECK_ARG(imgs && out && n_img >= 1 && n_img <= 65535 && n_inst >= 0 && (n_inst == 0 || kind));
    MPN_CHECK_ARG(max_w >= 1 && max_w <= 65536 && max_h >= 1 && max_h <= 65536 && out_bytes >= 1 && out_bytes <= (1L << 40));
    MPN_CHECK_ARG((uintptr_t)imgs % 8 == 0 && (uintptr_t)kind % 4 == 0);
    hipStream_t st = (hipStream_t)stream;
    const int rc = segm_toggle_stage(insts, n_inst, parts, n_parts, verts, vpart, estart, n_verts, n_steps, toggles, n_tog, -1L, workspace,
                                     ws_bytes, st);
    if (rc != 0) return rc;
    dim3 grid((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 64 * SEG_KC - 1) / (64 * SEG_KC)), (unsigned)n_img);
    if (out_all)
        hipLaunchKernelGGL(segm_mask_miss_kernel<true>, grid, dim3(256), 0, st, imgs, insts, n_inst, kind, parts, n_parts,
                           (const unsigned long long*)workspace, (long)(ws_bytes / 8), out, out_all, (long)out_bytes);
    else
        hipLaunchKernelGGL(segm_mask_miss_kernel<false>, grid, dim3(256), 0, st, imgs, insts, n_inst, kind, parts, n_parts,
                           (const unsigned long long*)workspace, (long)(ws_bytes / 8), out, (uint8_t*)nullptr, (long)out_bytes);
    return mpn_launch_status();
}

extern "C" int mpn_segm_mask_miss(const int64_t* imgs, int n_img, const int64_t* insts, const int32_t* kind, int n_inst, const int64_t* parts,
                                  int n_parts, const int32_t* verts, const int32_t* vpart, const int32_t* estart, int n_verts, int64_t n_steps,
                                  const int32_t* toggles, int n_tog, int max_w, int max_h, uint8_t* out, int64_t out_bytes, void* workspace,
                                  int64_t ws_bytes, void* stream) {
    return segm_compose(imgs, n_img, insts, kind, n_inst, parts, n_parts, verts, vpart, estart, n_verts, n_steps, toggles, n_tog, max_w,
                        max_h, out, nullptr, out_bytes, workspace, ws_bytes, stream);
}

extern "C" int mpn_segm_person_masks(const int64_t* imgs, int n_img, const int64_t* insts, const int32_t* kind, int n_inst,
                                     const int64_t* parts, int n_parts, const int32_t* verts, const int32_t* vpart, const int32_t* estart,
                                     int n_verts, int64_t n_steps, const int32_t* toggles, int n_tog, int max_w, int max_h, uint8_t* out_miss,
                                     uint8_t* out_all, int64_t out_bytes, void* workspace, int64_t ws_bytes, void* stream) {
    // the two planes of an image lie at one offset of two buffers of out_bytes each: the buffers must not overlap
    MPN_CHECK_ARG(out_all && out_miss && out_bytes >= 1 && out_bytes <= (1L << 40));
    MPN_CHECK_ARG((out_all > out_miss ? out_all - out_miss : out_miss - out_all) >= out_bytes);
    return segm_compose(imgs, n_img, insts, kind, n_inst, parts, n_parts, verts, vpart, estart, n_verts, n_steps, toggles, n_tog, max_w,
                        max_h, out_miss, out_all, out_bytes, workspace, ws_bytes, stream);
}
