// conv3_wino_sres: the split-resident 3x3x3 conv with the x axis in Winograd F(2,3) form -- two thirds of the matrix work.
//
// The fp16x3 conv is bound by the matrix pipe (MFMA-busy 0.86, clock at the power wall: profiles/r03_sq_summary.md); what moves its time
// is removing MFMAs.  Along x an output pair (X, X+1) of a k3 correlation needs the four inputs d0..d3 = in[X-1 .. X+2] and, per
// (dz, dy, cin), SIX products; in Winograd's minimal form FOUR:
//     t0 = d0 - d2   t1 = d1 + d2   t2 = d2 - d1   t3 = d1 - d3            (input transform: +-1 only)
//     u0 = g0   u1 = (g0 + g1 + g2) / 2   u2 = (g0 - g1 + g2) / 2   u3 = g2 (weights: host, in double, before the fp16 split)
//     m_f = sum over (dz, dy, cin) of t_f u_f                               (four GEMMs with K = 9 Cin instead of one with K = 27 Cin)
//     out[X] = (m0 + m1) + m2       out[X+1] = (m1 - m2) - m3               (output transform: +-1 only)
// The t_f are sums of two 22-bit values, formed in fp32 and split into an fp16 pair again exactly like a stored activation, so each
// product keeps the fp16x3 precision; the error against fp64 grows ~1.3 x over the direct form and stays at fp32-conv level
// (scripts/study/winograd_x_error.py).  y and z stay direct: each transformed axis doubles the accumulators, and 2 x is what fits.
//
// Workgroup = NG cout groups of four waves, ONE workgroup per CU (it holds 100 KB of LDS).  Block = 4 z x 8 y x 8 x outputs = 128
// x pairs; wave w of a group owns frequency f = w: four 32-row tiles (one per z slice; row = 8 y x 4 pairs) x 64 couts = 128
// accumulators, the same register shape as conv3_igemm_sres -- and the same tap loop, with 9 taps (dz, dy) per 16-channel chunk.
//
// Per chunk:  [transform: raw halo (LDS) -> T (LDS), one (z, y, pair, channel-half) unit per thread: 8 x 16 B in, ~180 VALU, 8 x 16 B out]
//             [barrier] [9 taps: A fragments from T, weight fragments from L2, 24 MFMAs each; the raw halo of chunk c+1 arrives by
//             LDS-DMA meanwhile, one piece per tap] [barrier].
// The raw halo (6 x 10 x 10 records) is single-buffered: it is dead once transformed, i.e. before the taps start.  T holds the four
// frequencies of the halo box: record (hz, f, hy, pair) at ((hz * 4 + f) * 10 + hy) * 4 + pair, slots XOR-swizzled by ((hy * NP + pair) >> 2) & 3
// (= hy & 3 for the main shape: 16 lanes of an A-fragment read = 4 y x 4 pairs hit 16 different 16-byte bank groups).  The raw box is laid out for the transform's
// reads, not as records: piece L = (hz * 10 + hy) * 41 + (term * 10 + hx) * 2 + half (one pad piece per row: 16 lanes = 4 y x 4 pairs
// read 16 different bank groups); global_load_lds writes lane-linearly, so the permutation is applied to the SOURCE address.
//
// Epilogue: the four frequencies of an output sit in four waves.  Per cout half the waves of a group exchange accumulators through
// LDS (wave w keeps z slice w: it sends three slices and receives three frequencies, 48 KB per group), apply the output transform,
// scale / shift / ReLU / split as conv3_igemm_sres does, build the block's image in LDS and copy it out 16 B per lane; ec3 / ec5:
// MaxPool3d(2) from that image (main shape, whole-tile boxes).  A transformed input beyond fp16's range turns its outputs NaN: the
// outputs inside the box are tested for finiteness before the ReLU and raise the overflow bit of the range flag.
//
// Measured (profiles/r03_winograd.md): 0.76-0.82 of the direct kernel's time per layer at 128 couts per workgroup, nothing at 64; what
// is left is the weight-fragment stream (36 / 27 of the direct form's bytes for 2 / 3 of its MFMAs) at the power wall.
//
// Every value of an output depends only on the parity of its x (pairs start at even tile coordinates: the host aligns the launch box)
// -- not on the block grid, the batch or the launch box: results do not depend on how tiles are batched.
#pragma once
#include "unet_sres2.h"
namespace oai {

// Block shapes: TY rows x NP pairs with TY * NP = 32 -- 8 x 4 (the main shape, figures above), 4 x 8 (y remainders of <= 4 rows) and
// 16 x 2 (x remainders of <= 4 columns): trimmed boxes are e.g. 12 x 52 x 52, and a block that is half outside its box costs all of its MFMAs.
// MS = 2 (NG = 1, layers with ONE block of 64 couts): eight waves all the same, wave (zp, f) owns frequency f of the z slices 2 zp, 2 zp + 1
// -- two accumulator tiles x 64 couts; the two waves of a frequency fetch the same weight fragments (the second from L1).  Four waves with
// four tiles each (NG = 1, MS = 1) leave every SIMD with one wave: measured no faster than the direct kernel.
// WS (NG = 1, MS = 1; one block of 64 couts): the eight waves are SPECIALISED.  Waves 0-3 only multiply -- wave = frequency, four tiles x 64
// couts per weight fragment set, the register shape of the two-group form -- and waves 4-7 only stage: each owns a quarter of the halo rows,
// requests their pieces, transforms them into the OTHER of two T buffers while the multipliers work on the current one, and requests the next
// chunk's pieces into the same places (no wave ever reads what another wave's DMA writes: no barrier inside the staging).  One barrier per
// chunk; no transform phase and no halo piece in front of a weight fragment on the multipliers' path.  2 x 60 KB of T + 40 KB of raw rows =
// the CU's 160 KB exactly.  (MS = 2 measured 0.43 MFMA-busy on dc2: its vector-memory path carries every weight fragment twice.)
// M16 (round 4; NG = 2, MS = 1, not WS): the same block, staging, transform and epilogue with the taps on v_mfma_f32_16x16x32_f16 instead of
// 32x32x16.  Why: this loop runs at the power wall, and at equal cycles per FLOP the 16x16x32 shape holds a ~12 % higher clock on split-fp16
// data with the structure of this tap loop (scripts/micro/mfma_shape.hip, profiles/r04_wino_stream.md: 1.66 -> 1.86 GHz, 1309 -> 1465 TFLOP/s
// executed at the same MFMA-busy share).  K = 32 is a PAIR OF TAPS x 16 channels, so every operand is a natural record read / panel load:
//     step j < 4:  taps (2j, 2j+1);  lanes 0-31 carry tap 2j, lanes 32-63 tap 2j+1 (lane group g = lane >> 4: channel half g & 1, tap g >> 1)
//         pass A  [a0(t) | a0(t')] . X'   X' = [b0(t) | b0(t')]        pass B  [a0 | a0'] . Y'   Y' = [b1(t) | b1(t')]        pass C  [a1 | a1'] . X'
//     step 4:      the ninth tap alone -- lanes 32-63 carry its LOW terms:  pass A  [a0 | a1] . [b0 | b0] = a0.b0 + a1.b0;  pass B  [a0 | a1] . [b1 | 0]
// = 14 K-32 MFMA steps per chunk where 13.5 would be exact (+3.7 %).  A wave's tile is the same 128 rows x 64 couts as 8 x 4 tiles of 16 x 16
// (m2 = 2 m + p: rows 16 p .. 16 p + 15 of slice m; n2 = 2 n + q): the same 128 accumulator registers, element (p, q, i) of the old (m, n)
// tile at row 16 p + 4 (lane >> 4) + i, cout column 16 q + (lane & 15).  Weight fragments: pack_wino16_panel, 40 KiB per chunk and 64 couts
// (36 in the 32x32 form), X' double-buffered, Y' reloaded behind pass B: 48 registers.  Every accumulator sees a0.b0 (two taps at once),
// a0.b1, a1.b0 per step: another summation order than the 32x32 form's, same arithmetic class (tests: the Winograd gates).
// (A persistent form of the WS kernel -- one workgroup per CU pulling blocks from per-XCD counters, the staging one block ahead -- was measured
// bit-identical and without gain, and removed: profiles/r05_persistent.md.)

// bytes of LDS of the instantiation <NG, TY, NP, MS, WS> (either tap form): the T buffer(s) + the raw box, as the body lays them out (it asserts the equality)
constexpr int wino_lds_bytes(int NG, int TY, int NP, int MS, bool WS) {
    const int NT = 256 * NG * MS, HZ = 6, HY = TY + 2, HX = 2 * NP + 2, RS = 4 * HX + 1;
    const int NIT = (HZ * HY * RS + NT - 1) / NT, TB = HZ * 4 * HY * NP * 64, WNIT = (HZ * HY / 4 * RS + 63) / 64;
    return (WS ? 2 : 1) * TB + (WS ? 4 * WNIT * 1024 : NIT * NT * 16);
}

// (The kernel's body is unet_wino_body.h: the one-launch kernels below run the same text on the blocks of their list.)
template <int NG, int TY, int NP, int MS = 1, bool WS = false, bool M16 = false>
__global__ void __launch_bounds__(WS ? 512 : 256 * NG * MS, 1) conv3_wino_sres(const ConvArgs a, const unsigned char* __restrict__ zero_rec) {
#include "unet_wino_body.h"
}

// ---- option "one_launch": one launch per own-cover layer over the batch's LIVE-BLOCK LIST
// With option "own_cover" a trimmed decoder layer is three launches, one per block shape over every tile's own cover, each with the grid of the batch's
// largest tile.  The three are independent, but one stream runs them one after the other: every strip launch pays a whole last round of the chip for a
// few hundred workgroups (profiles/own_cover.md: 10.8 ms of strips per 160-tile pass), and a smaller tile's surplus workgroups start only to return.
// A strip block is the same MFMA count as a main block -- what differs is the launch.  So the one-launch kernels below take ONE grid over a device list
// of the batch's live blocks (block_list_kernel in unet.hip: all main blocks in tile order, then the x strips, then the y strips; no dead entry), read
// their entry, and branch -- once, workgroup-uniform, before any load -- into the body of the entry's shape: the strips fill the main blocks' last round
// and the layer pays one tail.  The bodies are the stand-alone kernels' own text (unet_wino_body.h), called with the listed block: a block's arithmetic
// and its bits do not depend on which launch runs it.
//
// A list entry is one word, wino_list_entry: tile (index in the batch) << 20 | shape << 18 | bz << 12 | by << 6 | bx -- shape 0 main (8 x 8), 1 x strip
// (16 x 4), 2 y strip (4 x 16); (bz, by, bx) count from the tile's own piece row, as with ConvArgs::own_origin.  The host takes the three-launch path
// for a batch whose counts do not fit the fields.  Workgroup id -> (list index, cout block) as in the stand-alone kernels: id % ncb is the cout
// block, and xcd_block_id deals the ids -- of live blocks only, so the XCDs' shares are equal to one deal.
// ConvArgs of a one-launch kernel: reserved1 = the list, nblocks = entries x ncb, boxes = the piece rows of shape 0 and nbz = the distance in ints to the
// rows of the next shape (the table of box_table_kernel: consecutive rows); nby, nbx unused; lo / hi = the whole level, own_origin = 1.
constexpr int kWinoListTileBits = 12, kWinoListAxisBits = 6;
__host__ __device__ constexpr unsigned wino_list_entry(int tile, int shape, int bz, int by, int bx) {
    return (unsigned)tile << 20 | (unsigned)shape << 18 | (unsigned)bz << 12 | (unsigned)by << 6 | (unsigned)bx;
}

template <int NG, int TY, int NP, int MS, bool WS, bool M16, int LDSB>
__device__ __forceinline__ void conv3_wino_block(const ConvArgs& a, const unsigned char* __restrict__ zero_rec, unsigned char* const lds, const int* l_boxes,
                                                 int l_tile, int l_bz, int l_by, int l_bx, int l_cbg) {
#define OAI_WINO_LISTED 1
#include "unet_wino_body.h"
#undef OAI_WINO_LISTED
}

// this workgroup's list entry and cout block; false for the padding of the XCD dealing
__device__ __forceinline__ bool wino_list_block(const ConvArgs& a, unsigned& entry, int& cbg) {
    int id = a.xcd_group ? xcd_block_id(a.nblocks, a.xcd_group) : (int)blockIdx.x;
    if (id < 0) return false;
    cbg = id % a.ncb; id /= a.ncb;
    entry = (unsigned)__builtin_amdgcn_readfirstlane(a.reserved1[id]);
    return true;
}
constexpr int imax3(int x, int y, int z) { return x > y ? (x > z ? x : z) : (y > z ? y : z); }

// the two-group form (layers with Cout % 128 == 0: dc8, dc7, dc5, dc4), either tap form
template <bool M16>
__global__ void __launch_bounds__(512, 1) conv3_wino_list2(const ConvArgs a, const unsigned char* __restrict__ zero_rec) {
    constexpr int LDSB = imax3(wino_lds_bytes(2, 8, 4, 1, false), wino_lds_bytes(2, 16, 2, 1, false), wino_lds_bytes(2, 4, 8, 1, false));
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDSB];
    unsigned e;
    int cbg;
    if (!wino_list_block(a, e, cbg)) return;
    const int shape = (e >> 18) & 3, tile = e >> 20, bz = (e >> 12) & 63, by = (e >> 6) & 63, bx = e & 63;
    const int* boxes = a.boxes + (size_t)shape * a.nbz;
    if (shape == 0) conv3_wino_block<2, 8, 4, 1, false, M16, LDSB>(a, zero_rec, lds, boxes, tile, bz, by, bx, cbg);
    else if (shape == 1) conv3_wino_block<2, 16, 2, 1, false, M16, LDSB>(a, zero_rec, lds, boxes, tile, bz, by, bx, cbg);
    else conv3_wino_block<2, 4, 8, 1, false, M16, LDSB>(a, zero_rec, lds, boxes, tile, bz, by, bx, cbg);
}

// the 64-cout form (dc2): specialised waves for the main blocks and the x strip, the slice-split form for the y strip (whose two T buffers would not fit),
// as launch_wino_shape picks them; either tap form
template <bool M16>
__global__ void __launch_bounds__(512, 1) conv3_wino_list1(const ConvArgs a, const unsigned char* __restrict__ zero_rec) {
    constexpr int LDSB = imax3(wino_lds_bytes(1, 8, 4, 1, true), wino_lds_bytes(1, 16, 2, 1, true), wino_lds_bytes(1, 4, 8, 2, false));
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDSB];
    unsigned e;
    int cbg;
    if (!wino_list_block(a, e, cbg)) return;
    const int shape = (e >> 18) & 3, tile = e >> 20, bz = (e >> 12) & 63, by = (e >> 6) & 63, bx = e & 63;
    const int* boxes = a.boxes + (size_t)shape * a.nbz;
    if (shape == 0) conv3_wino_block<1, 8, 4, 1, true, M16, LDSB>(a, zero_rec, lds, boxes, tile, bz, by, bx, cbg);
    else if (shape == 1) conv3_wino_block<1, 16, 2, 1, true, M16, LDSB>(a, zero_rec, lds, boxes, tile, bz, by, bx, cbg);
    else conv3_wino_block<1, 4, 8, 2, false, M16, LDSB>(a, zero_rec, lds, boxes, tile, bz, by, bx, cbg);
}

}  // namespace oai
