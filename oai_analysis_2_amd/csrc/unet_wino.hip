// The Winograd F(2,3) k3 conv kernels and their launchers: conv3_wino_sres, conv3_wino_list1 / conv3_wino_list2, conv3_wino_f32.
// No other file names these kernels: their instantiations are emitted here.
#include "unet_host.h"
#include "unet_wino.h"
#include "unet_wino_f32.h"

namespace oai {

// The specialised 64-cout form takes ALL of a CU's LDS (160 KB): asked once whether a workgroup of it (both block shapes, both tap forms) fits this
// device / driver at all
static bool wino_ws_fits() {
    static const bool fits = [] {
        auto one = [](auto kern) { int n = 0; return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 512, 0) == hipSuccess && n >= 1; };
        return one(conv3_wino_sres<1, 8, 4, 1, true>) && one(conv3_wino_sres<1, 16, 2, 1, true>) &&
               one(conv3_wino_sres<1, 8, 4, 1, true, true>) && one(conv3_wino_sres<1, 16, 2, 1, true, true>);
    }();
    return fits;
}
// a 64-cout layer on the 16x16x32 taps (option "winograd" bit 5): its main blocks and x strip run the specialised form's tap-pair variant, its y strip
// the slice-split form's -- ALL its launch shapes or none: a voxel's bits must not depend on which shape covers it
static bool wino_m16_64(const oai_unet* h, const Layer& L, int cout) {
    return cout % 128 != 0 && (h->opt_wino & 32) && !(h->opt_wino & (4 | 8)) && L.panel_wino16 && wino_ws_fits();
}

// cout groups of 64 per workgroup of conv3_wino_sres for a layer and a block height
int wino_groups(const oai_unet* h, int cout, int TY) {
    return (cout % 128 == 0 && !((h->opt_wino & 8) && TY != 4)) ? 2 : 1;      // (bit 3, A/B: the specialised 64-cout form for every layer)
}
// One launch of conv3_wino_sres (unet_wino.h) with blocks of 4 x TY x 2 NP over `box` (box.lo[2] even)
template <int TY, int NP>
static int launch_wino_shape(const oai_unet* h, const Layer& L, ConvArgs a, const Box& box, int ntiles, hipStream_t st, const int* own_nb = nullptr, int own_group = 0) {
    for (int i = 0; i < 3; ++i) { a.lo[i] = box.lo[i]; a.hi[i] = box.hi[i]; }
    if (box.hi[0] <= box.lo[0] || box.hi[1] <= box.lo[1] || box.hi[2] <= box.lo[2]) return OAI_OK;
    a.own_origin = own_nb != nullptr;                                  // (own_nb: a.boxes = one piece of every tile's own cover, the grid counted from each row's start)
    const int ng = wino_groups(h, a.Cout, TY);
    a.wpanel = L.panel_wino;
    a.ncb = a.Cout / (64 * ng);
    a.nbz = cdiv(box.hi[0] - box.lo[0], 4); a.nby = cdiv(box.hi[1] - box.lo[1], TY); a.nbx = cdiv(box.hi[2] - box.lo[2], 2 * NP);
    if (own_nb) { a.nbz = own_nb[0]; a.nby = own_nb[1]; a.nbx = own_nb[2]; }
    unsigned grid = (unsigned)((size_t)ntiles * a.nbz * a.nby * a.nbx * a.ncb);
    grid = xcd_deal(h, grid, a.nblocks, a.xcd_group, own_group);
    if (int rc = launch_begin(h, st)) return rc;
    if (ng == 2 && (h->opt_wino & 16) && L.panel_wino16) {              // the taps on v_mfma_f32_16x16x32_f16 (higher clock at the power wall)
        a.wpanel = L.panel_wino16;
        conv3_wino_sres<2, TY, NP, 1, false, true><<<grid, 512, 0, st>>>(a, h->zero_rec);
    } else if (ng == 2) conv3_wino_sres<2, TY, NP><<<grid, 512, 0, st>>>(a, h->zero_rec);
    else if constexpr (TY != 4) {
        if ((h->opt_wino & 4) || !wino_ws_fits()) conv3_wino_sres<1, TY, NP, 2><<<grid, 512, 0, st>>>(a, h->zero_rec);        // (A/B, or no room: the eight waves split the z slices)
        else if (wino_m16_64(h, L, a.Cout)) {                                                          // the multipliers' taps on v_mfma_f32_16x16x32_f16
            a.wpanel = L.panel_wino16;
            conv3_wino_sres<1, TY, NP, 1, true, true><<<grid, 512, 0, st>>>(a, h->zero_rec);
        } else conv3_wino_sres<1, TY, NP, 1, true><<<grid, 512, 0, st>>>(a, h->zero_rec);              // one block of 64 couts: four waves multiply, four stage
    } else if (wino_m16_64(h, L, a.Cout)) {                                          // (the y strip's two T buffers would not fit: the eight waves split the z slices --
        a.wpanel = L.panel_wino16;                                                     //  on the same tap pairs as the layer's other shapes: one summation order per layer)
        conv3_wino_sres<1, TY, NP, 2, false, true><<<grid, 512, 0, st>>>(a, h->zero_rec);
    } else conv3_wino_sres<1, TY, NP, 2><<<grid, 512, 0, st>>>(a, h->zero_rec);
    return launch_end(h, st);
}

// Which one-launch kernel an own-cover layer takes (option "one_launch"): 1 = conv3_wino_list2 (two cout groups), 2 = conv3_wino_list1 (one block of 64
// couts), 0 = none -- the option's bit is off, or the configuration gives the layer's shapes kernels that these two do not combine (the A/B bits 2 and 3
// of option "winograd", no room for the specialised form)
int one_launch_family(const oai_unet* h, const Layer& L) {
    if (L.cout % 128 == 0) return (h->opt_one_launch & 1) && !(h->opt_wino & 8) ? 1 : 0;
    return (h->opt_one_launch & 2) && L.cout % 64 == 0 && !(h->opt_wino & 4) && wino_ws_fits() ? 2 : 0;
}
// The size gate of option "one_launch": the entries of the layer's list, or 0 = three launches for this batch.  Without the force bit a layer runs as one
// launch only when its live blocks number at least the device's CUs: below that the three launches are not even one round of the chip and there is no tail
// to save -- and the launch structure of small batches is pinned by the tests (tests/test_unet_gpu.py counts the timed launches of batches of 9 tiles).
// Small batches are not what the library is timed on.
int one_launch_len(const oai_unet* h, const int* tile_nb, int ntiles, int slot, size_t capacity) {
    static const int cus = [] { int dev = 0, n = 0; return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess ? n : 1 << 30; }();
    const int len = block_list_len(tile_nb, ntiles, slot, capacity);
    return (h->opt_one_launch & 4) || len >= cus ? len : 0;
}
// One own-cover layer as ONE launch of conv3_wino_list2 / conv3_wino_list1 over its live-block list (option "one_launch"; unet_wino.h says what the kernels
// read of ConvArgs); `level` = the whole level, as for the three launches.  One launch = one start / stop pair of oai_unet_profile.
static int launch_wino_list(const oai_unet* h, const Layer& L, ConvArgs a, const Box& level, hipStream_t st, const OwnCover& oc, int family) {
    for (int i = 0; i < 3; ++i) { a.lo[i] = level.lo[i]; a.hi[i] = level.hi[i]; }
    a.own_origin = 1;
    a.boxes = oc.rows[0]; a.nbz = (int)(oc.rows[1] - oc.rows[0]); a.nby = a.nbx = 0;      // the piece rows of the three shapes are equally spaced table rows
    a.reserved1 = reinterpret_cast<int*>(const_cast<unsigned*>(oc.list));
    a.ncb = a.Cout / (family == 1 ? 128 : 64);
    const unsigned grid = xcd_deal(h, (unsigned)((size_t)oc.list_len * a.ncb), a.nblocks, a.xcd_group);      // only live blocks are dealt: the option's granularity balances
    const bool m16 = family == 1 ? (h->opt_wino & 16) && L.panel_wino16 : wino_m16_64(h, L, a.Cout);          // (the tap form that launch_wino_shape picks for the layer)
    a.wpanel = m16 ? L.panel_wino16 : L.panel_wino;
    if (int rc = launch_begin(h, st)) return rc;
    if (family == 1) {
        if (m16) conv3_wino_list2<true><<<grid, 512, 0, st>>>(a, h->zero_rec);
        else conv3_wino_list2<false><<<grid, 512, 0, st>>>(a, h->zero_rec);
    } else {
        if (m16) conv3_wino_list1<true><<<grid, 512, 0, st>>>(a, h->zero_rec);
        else conv3_wino_list1<false><<<grid, 512, 0, st>>>(a, h->zero_rec);
    }
    return launch_end(h, st);
}

// A plain layer (no fused ec0 / pool / head / scatter) of the default split-resident configuration through conv3_wino_sres: main blocks of
// 4 x 8 x 8, a y strip of 4 x 4 x 16 blocks for a remainder of <= 4 rows, an x strip of 4 x 16 x 4 blocks for a remainder of <= 4 columns
// .  The box starts at an even x: an output's arithmetic depends on the
// parity of its x only -- not on which launch or block computes it.
// `oc` (option "own_cover"; the trimmed decoder layers of oai_segment_tiles): the same three shapes, one launch each, over every tile's OWN cover
// (tile_cover) instead of the cover of the batch's union box: a border tile's blocks start at its own corner, and its own remainders decide its
// strips.  The launch box is the whole level; a shape that no tile of the batch needs is not launched.  Same bits.  With a live-block list (option
// "one_launch") the three launches are one: launch_wino_list.
int launch_conv3_wino(const oai_unet* h, const Layer& L, const ConvArgs& a, Box box, int ntiles, hipStream_t st, const OwnCover* oc) {
    if (oc && a.boxes) {
        const int dims[3] = {a.D, a.H, a.W};
        Box level;
        full_box(level, dims);
        if (oc->list_len > 0)
            if (const int family = one_launch_family(h, L)) return launch_wino_list(h, L, a, level, st, *oc, family);
        ConvArgs b = a;
        for (int s = 0; s < 3; ++s) {
            if (oc->nb[s][0] == 0) continue;
            b.boxes = oc->rows[s];
            const int rc = s == 0 ? launch_wino_shape<8, 4>(h, L, b, level, ntiles, st, oc->nb[s], oc->xcd_group[s])
                         : s == 1 ? launch_wino_shape<16, 2>(h, L, b, level, ntiles, st, oc->nb[s], oc->xcd_group[s])
                                  : launch_wino_shape<4, 8>(h, L, b, level, ntiles, st, oc->nb[s], oc->xcd_group[s]);
            if (rc) return rc;
        }
        return OAI_OK;
    }
    box.lo[2] &= ~1;
    const Cover c = cover_box(box, 8, 4, 4, false);
    if (int rc = launch_wino_shape<8, 4>(h, L, a, c.main, ntiles, st)) return rc;
    if (c.wr)
        if (int rc = launch_wino_shape<16, 2>(h, L, a, c.xs, ntiles, st)) return rc;
    if (c.hr)
        if (int rc = launch_wino_shape<4, 8>(h, L, a, c.ys, ntiles, st)) return rc;
    return OAI_OK;
}

// the fused max-pool of conv3_wino_sres pools whole 2 x 2 x 2 windows of a block's own image: the box must be the whole (even-sized) tile
// level, so that every block (any shape) starts at even coordinates and lies inside it
bool wino_pool_box(const Box& box, const int dims[3]) {
    for (int i = 0; i < 3; ++i)
        if (box.lo[i] != 0 || box.hi[i] != dims[i] || (dims[i] & 1)) return false;
    return dims[0] % 4 == 0 && dims[1] % 8 == 0 && dims[2] % 8 == 0;      // main blocks only: no strips
}

// One launch of conv3_wino_f32 (unet_wino_f32.h) with blocks of 2 x TY x 2 NP over `box` (box.lo[2] even)
template <int TY, int NP>
static int launch_wino_f32_shape(const oai_unet* h, const Layer& L, ConvArgs a, const Box& box, int ntiles, hipStream_t st) {
    for (int i = 0; i < 3; ++i) { a.lo[i] = box.lo[i]; a.hi[i] = box.hi[i]; }
    if (box.hi[0] <= box.lo[0] || box.hi[1] <= box.lo[1] || box.hi[2] <= box.lo[2]) return OAI_OK;
    a.wpanel = L.panel_wino_f32;
    a.ncb = (a.Cout + 63) / 64;
    a.nbz = cdiv(box.hi[0] - box.lo[0], 2); a.nby = cdiv(box.hi[1] - box.lo[1], TY); a.nbx = cdiv(box.hi[2] - box.lo[2], 2 * NP);
    unsigned grid = (unsigned)((size_t)ntiles * a.nbz * a.nby * a.nbx * a.ncb);
    grid = xcd_deal(h, grid, a.nblocks, a.xcd_group);         // (as the split-resident kernels)
    if (int rc = launch_begin(h, st)) return rc;
    conv3_wino_f32<TY, NP><<<grid, 256, 0, st>>>(a, reinterpret_cast<const float*>(h->zero_rec));
    return launch_end(h, st);
}

// The exact-fp32 path's k3 layers through conv3_wino_f32: main blocks of 2 x 8 x 8, a y strip of 2 x 4 x 16 blocks for a remainder of <= 4 rows, an x strip
// of 2 x 16 x 4 blocks for a remainder of <= 4 columns (the cover of launch_conv3_wino).  The box starts at an even x: an output's arithmetic depends on the
// parity of its x only -- not on which launch or block computes it.  A fused MaxPool3d(2) rides in the main blocks (the host passes it for whole-tile boxes only).
int launch_conv3_wino_f32(const oai_unet* h, const Layer& L, const ConvArgs& a, Box box, int ntiles, hipStream_t st) {
    box.lo[2] &= ~1;
    const Cover c = cover_box(box, 8, 4, 4, a.pool_out != nullptr);
    if (int rc = launch_wino_f32_shape<8, 4>(h, L, a, c.main, ntiles, st)) return rc;
    if (c.wr)
        if (int rc = launch_wino_f32_shape<16, 2>(h, L, a, c.xs, ntiles, st)) return rc;
    if (c.hr)
        if (int rc = launch_wino_f32_shape<4, 8>(h, L, a, c.ys, ntiles, st)) return rc;
    return OAI_OK;
}

}  // namespace oai
