// Host side of the segmentation path: tile geometry and workspace planning, the layer schedule of UNet.forward
// (networks.py:109-149) with the bit-identical dead-output trim, the options and the C ABI.
// Weight ingest is unet_pack.hip; the launchers of the kernel families are in unet_direct.hip (+ unet_direct_m16.hip),
// unet_wino.hip and unet_small.hip (unet_host.h); the two kernels here build the box table and the block lists.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

#include "unet_host.h"
#include "unet_wino.h"      // the entry format of the live-block lists (wino_list_entry); no kernel of it is named here

#ifdef OAI_DIAG
static unsigned long long* g_diag_stamps = nullptr;
static unsigned long long* diag_stamps() {
    if (!g_diag_stamps && oai::diag_env("OAI_STAMPS", 0)) {
        if (hipMalloc((void**)&g_diag_stamps, 32 * sizeof(unsigned long long)) != hipSuccess) return nullptr;
        (void)hipMemset(g_diag_stamps, 0, 32 * sizeof(unsigned long long));
    }
    return g_diag_stamps;
}
extern "C" int oai_diag_stamps(unsigned long long out[32], int reset) {      // diagnostic builds only (not in include/oai_hip.h)
    if (!g_diag_stamps) return 1;
    if (hipMemcpy(out, g_diag_stamps, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    if (reset) (void)hipMemset(g_diag_stamps, 0, 32 * sizeof(unsigned long long));
    return 0;
}
#endif

namespace oai {

// Output box each layer must produce so that the kept centre is unchanged (oracle/seg.py:trim_regions)
__host__ __device__ static void plan_regions(const int tile[3], const int keep_lo[3], const int keep_hi[3], bool trimmed, Box need[18]) {
    int dims[4][3];
    for (int l = 0; l < 4; ++l) for (int i = 0; i < 3; ++i) dims[l][i] = tile[i] >> l;
    for (int k = 0; k < 18; ++k) full_box(need[k], dims[layer_level(k)]);
    for (int i = 0; i < 3; ++i) { need[DC0].lo[i] = keep_lo[i]; need[DC0].hi[i] = keep_hi[i]; }   // the head always crops
    if (!trimmed) return;
    auto grow = [&](const Box& b, int lvl) { Box r; for (int i = 0; i < 3; ++i) { r.lo[i] = b.lo[i] > 0 ? b.lo[i] - 1 : 0; r.hi[i] = b.hi[i] + 1 < dims[lvl][i] ? b.hi[i] + 1 : dims[lvl][i]; } return r; };
    auto halve = [&](const Box& b) { Box r; for (int i = 0; i < 3; ++i) { r.lo[i] = b.lo[i] / 2; r.hi[i] = (b.hi[i] + 1) / 2; } return r; };
    Box keep; for (int i = 0; i < 3; ++i) { keep.lo[i] = keep_lo[i]; keep.hi[i] = keep_hi[i]; }
    need[DC0] = keep; need[DC1] = keep;
    need[DC2] = grow(need[DC1], 0);
    need[DC3] = grow(need[DC2], 0);
    need[DC4] = halve(need[DC3]);
    need[DC5] = grow(need[DC4], 1);
    need[DC6] = grow(need[DC5], 1);
    need[DC7] = halve(need[DC6]);
    need[DC8] = grow(need[DC7], 2);
    // dc9 and the encoder stay full: the bottleneck sees the whole tile
}

constexpr int kMaxTilesPerTable = 4096;
// The layers whose blocks sit on every tile's OWN cover (option "own_cover"): the trimmed decoder convs.  After the 18 box rows of a tile the table holds
// three more rows per such layer, one per block shape (tile_cover): rows 18 + 3 slot + shape, addressed like the layers' own.
constexpr int kTableRows = 18 + 3 * kOwnLayers;
__host__ __device__ static inline int own_cover_slot(int k) { return k == DC8 ? 0 : k == DC7 ? 1 : k == DC5 ? 2 : k == DC4 ? 3 : k == DC2 ? 4 : -1; }
constexpr int kOwnLayerOf[kOwnLayers] = {DC8, DC7, DC5, DC4, DC2};

// The workspace of one pass of `batch` tiles: the per-tile box table of the current oai_segment_tiles call at the start, then the activation
// tensors.  Returns the bytes; over a null `base` the pointers are null and only the size counts (oai::Ws).
// entries that the live-block list of ONE own-cover layer can have for a batch (option "one_launch"): every layer gets the room of a whole tile at level 0
// -- main blocks of 4 x 8 x 8, one column of x-strip blocks, one row of y-strip blocks (the x start rounded down to even may add a block column)
static size_t block_list_capacity(int td, int th, int tw, int batch) {
    return (size_t)batch * cdiv(td, 4) * ((size_t)cdiv(th, 8) * cdiv(tw + 1, 8) + cdiv(th, 16) + cdiv(tw + 1, 16));
}
// where the list of own-cover layer `slot` starts in the workspace, in bytes: behind the box table, one list after the other.  (Depends on the tile
// shape and the batch only: oai_unet_block_list reports it without a handle.)
static size_t block_list_offset(int td, int th, int tw, int batch, int slot) {
    return round256((size_t)kTableRows * kMaxTilesPerTable * 6 * sizeof(int)) + slot * round256(block_list_capacity(td, th, tw, batch) * sizeof(unsigned));
}

static size_t carve_workspace(const oai_unet* h, int td, int th, int tw, int batch, const void* base, float* buf[B_COUNT], int*& table, unsigned** lists = nullptr) {
    const size_t v0 = (size_t)td * th * tw, v1 = v0 / 8, v2 = v1 / 8, v3 = v2 / 8;
    const oai::Layer* L = h->L;
    auto pc = [&](int k) { return (size_t)((L[k].cout + 15) / 16 * 16); };   // channels padded to whole 16-chunks (format S)
    const size_t sizes[B_COUNT] = {
        v0 * pc(EC0), v0 * pc(EC1), v1 * pc(EC1), v1 * pc(EC2), v1 * pc(EC3), v2 * pc(EC3),
        v2 * pc(EC4), v2 * pc(EC5), v3 * pc(EC5), v3 * pc(EC6), v3 * pc(EC7), v2 * pc(DC9),
        v2 * pc(DC8), v2 * pc(DC7), v1 * pc(DC6), v1 * pc(DC5), v1 * pc(DC4), v0 * pc(DC3),
        v0 * pc(DC2), v0 * pc(DC1)};
    Ws ws(base);
    table = ws.take<int>((size_t)kTableRows * kMaxTilesPerTable * 6);
    for (int slot = 0; slot < kOwnLayers; ++slot) {                    // (block_list_offset says where these are)
        unsigned* list = ws.take<unsigned>(block_list_capacity(td, th, tw, batch));
        if (lists) lists[slot] = list;
    }
    for (int i = 0; i < B_COUNT; ++i) buf[i] = ws.take<float>(sizes[i] * batch);
    return ws.off;
}
static size_t workspace_bytes(const oai_unet* h, int td, int th, int tw, int batch) {
    float* buf[B_COUNT];
    int* table;
    return carve_workspace(h, td, th, tw, batch, nullptr, buf, table);
}

// One timed launch: with profiling on (oai_unet_profile) the kernel sits between a start / stop pair of the handle's event pool, which grows as needed and
// is reused after every oai_unet_profile_read.  launch_begin before the launch; launch_end after it checks the launch and records the stop event.
int launch_begin(const oai_unet* h, hipStream_t st) {
    if (!h->profile) return OAI_OK;
    oai_unet* hm = const_cast<oai_unet*>(h);
    while (hm->ev_used + 2 > hm->ev_pool.size()) {
        hipEvent_t e;
        OAI_CHECK_HIP(hipEventCreate(&e));
        hm->ev_pool.push_back(e);
    }
    OAI_CHECK_HIP(hipEventRecord(hm->ev_pool[hm->ev_used], st));
    return OAI_OK;
}
int launch_end(const oai_unet* h, hipStream_t st) {
    OAI_CHECK_LAUNCH();
    if (!h->profile) return OAI_OK;
    oai_unet* hm = const_cast<oai_unet*>(h);
    OAI_CHECK_HIP(hipEventRecord(hm->ev_pool[hm->ev_used + 1], st));
    hm->ev_used += 2;
    return OAI_OK;
}

// XCD-aware dealing of a launch's logical block list (xcd_block_id in the kernels): the kernel gets the number of real blocks and the grid is rounded up
// to whole deals of xcd_group blocks to each of the 8 XCDs.  Option "xcd_group" 0: plain launch order, the grid as it is.
// `group` > 0: this launch's own granularity (balanced_xcd_group) instead of the option's.
unsigned xcd_deal(const oai_unet* h, unsigned grid, int& nblocks, int& xcd_group, int group) {
    if (h->xcd_group <= 0) return grid;
    nblocks = (int)grid; xcd_group = group > 0 ? group : h->xcd_group;
    const unsigned q = 8u * (unsigned)xcd_group;
    return (grid + q - 1) / q * q;
}

#ifdef OAI_DIAG
unsigned long long* layer_stamps(const oai_unet* h, const Layer& L) {    // OAI_STAMP_LAYER: one layer's budget (EC1 = 1 ..., DC9 = 8, DC6 = 11, DC3 = 14)
    static const int only = diag_env("OAI_STAMP_LAYER", -1);
    return only >= 0 && layer_id(h, L) != only ? nullptr : diag_stamps();
}
#endif

// The cover of ONE tile's own box by the shapes of launch_conv3_wino (option "own_cover"): piece[0] main blocks of 8 x 8, piece[1] the x strip (16 x 4),
// piece[2] the y strip (4 x 16) -- cover_box's rules on the box with its x start rounded down to even, which is where the tile's blocks start; the
// pieces themselves keep the true start, are disjoint and make up the box; a piece may be empty.  Host (grid sizes, oai_unet_cover_stats) and device
// (box_table_kernel) run this one function.
__host__ __device__ static void tile_cover(const Box& box, Box piece[3]) {
    Box even = box;
    even.lo[2] &= ~1;
    const Cover c = cover_box(even, 8, 4, 4, false);
    piece[0] = c.main; piece[1] = c.xs; piece[2] = c.ys;
    piece[0].lo[2] = piece[2].lo[2] = box.lo[2];
}
constexpr int kWinoTY[3] = {8, 16, 4}, kWinoTX[3] = {8, 4, 16};         // the block shapes of the three pieces (4 z slices each)
// blocks of shape `s` that piece `p` of a tile takes from its own origin (0 0 0: empty piece)
__host__ __device__ static void piece_blocks(const Box& p, int s, int nb[3]) {
    nb[0] = nb[1] = nb[2] = 0;
    if (box_empty(p)) return;
    const int ty = s == 0 ? 8 : s == 1 ? 16 : 4, tx = s == 0 ? 8 : s == 1 ? 4 : 16;      // (kWinoTY / kWinoTX: host arrays)
    nb[0] = (p.hi[0] - p.lo[0] + 3) / 4; nb[1] = (p.hi[1] - p.lo[1] + ty - 1) / ty; nb[2] = (p.hi[2] - (p.lo[2] & ~1) + tx - 1) / tx;
}
constexpr int kTileNbStride = kOwnLayers * 3 * 3;
static void own_plan_add(OwnPlan& op, const Box need[18]) {
    const size_t row = op.tile_nb.size();
    op.tile_nb.resize(row + kTileNbStride, 0);
    for (int k = 0; k < 18; ++k) {
        if (box_empty(need[k])) continue;
        if (layer_kind(k) == 2) {
            int v = 1;
            for (int i = 0; i < 3; ++i) v *= (need[k].hi[i] + 1) / 2 - need[k].lo[i] / 2;
            op.up_nvox[k] = std::max(op.up_nvox[k], v);
        }
        const int slot = own_cover_slot(k);
        if (slot < 0) continue;
        Box piece[3];
        tile_cover(need[k], piece);
        for (int s = 0; s < 3; ++s) {
            int nb[3];
            piece_blocks(piece[s], s, nb);
            for (int i = 0; i < 3; ++i) { op.nb[slot][s][i] = std::max(op.nb[slot][s][i], nb[i]); op.tile_nb[row + (slot * 3 + s) * 3 + i] = nb[i]; }
        }
    }
}

// ---- option "one_launch": the live-block list of an own-cover layer (unet_wino.h: conv3_wino_list*)
// Entries of layer `slot` for a batch whose tiles' block counts are `tile_nb` (OwnPlan): every live block of every piece once -- or 0 where a field does
// not fit the entry format (wino_list_entry) or the list its room in the workspace: that batch keeps its three launches.
int block_list_len(const int* tile_nb, int ntiles, int slot, size_t capacity) {
    if (ntiles > (1 << kWinoListTileBits)) return 0;
    long long len = 0;
    for (int t = 0; t < ntiles; ++t)
        for (int s = 0; s < 3; ++s) {
            const int* nb = tile_nb + (size_t)t * kTileNbStride + (slot * 3 + s) * 3;
            for (int i = 0; i < 3; ++i) if (nb[i] > (1 << kWinoListAxisBits)) return 0;
            len += (long long)nb[0] * nb[1] * nb[2];
        }
    return len <= (long long)capacity && len < (1ll << 30) ? (int)len : 0;
}
// The list in its order, on the host (oai_unet_block_list; the device builds the same with block_list_kernel): all main blocks -- tile by tile, a tile's
// blocks as the stand-alone launch numbers them, bx fastest -- then all x-strip blocks, then all y-strip blocks.  Hardware starts workgroups in id order:
// the strips run in the main blocks' last round.
static void block_list_host(const int* tile_nb, int ntiles, int slot, unsigned* out) {
    for (int s = 0; s < 3; ++s)
        for (int t = 0; t < ntiles; ++t) {
            const int* nb = tile_nb + (size_t)t * kTileNbStride + (slot * 3 + s) * 3;
            for (int bz = 0; bz < nb[0]; ++bz)
                for (int by = 0; by < nb[1]; ++by)
                    for (int bx = 0; bx < nb[2]; ++bx) *out++ = wino_list_entry(t, s, bz, by, bx);
        }
}
// The same list on the device, from the piece rows that box_table_kernel wrote for the batch's tiles [t0, t0 + n) of a table of table_tiles tiles: per
// (shape, tile) the block count (piece_blocks, the function the host counts with), ONE ordered exclusive scan over the 3 n counts in LDS -- every thread
// sums its consecutive share, a Hillis-Steele scan orders the 256 shares -- then entry e is found by bisection in the offsets.  No atomics: the list is
// the same in every run.  Workgroup = (layer slot, one of kListParts interleaved parts of the entries); every workgroup repeats the (cheap) scan.
constexpr int kListParts = 8;
__global__ void __launch_bounds__(256) block_list_kernel(const int* __restrict__ table, int table_tiles, int t0, int n, unsigned* __restrict__ lists, size_t stride,
                                                          int capacity, int slot_mask) {
    __shared__ int off[3 * kMaxTilesPerTable + 1];
    __shared__ int share[256];
    const int slot = blockIdx.x / kListParts, part = blockIdx.x % kListParts, tid = threadIdx.x;
    if (!((slot_mask >> slot) & 1)) return;
    auto blocks_of = [&](int item, int nb[3]) {
        const int s = item / n, t = item - s * n;
        const int* row = table + ((size_t)(18 + 3 * slot + s) * table_tiles + t0 + t) * 6;
        Box p;
        for (int i = 0; i < 3; ++i) { p.lo[i] = row[i]; p.hi[i] = row[3 + i]; }
        piece_blocks(p, s, nb);
    };
    const int items = 3 * n, per = (items + 255) / 256;
    for (int i = tid; i < items; i += 256) {
        int nb[3];
        blocks_of(i, nb);
        off[i] = nb[0] * nb[1] * nb[2];
    }
    __syncthreads();
    const int lo = min(items, tid * per), hi = min(items, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += off[i];
    share[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = tid >= d ? share[tid - d] : 0;
        __syncthreads();
        share[tid] += v;
        __syncthreads();
    }
    int run = share[tid] - sum;
    for (int i = lo; i < hi; ++i) { const int c = off[i]; off[i] = run; run += c; }
    if (tid == 255) off[items] = share[255];
    __syncthreads();
    const int total = min(off[items], capacity);                        // (the host launches this only for a list that fits: block_list_len)
    unsigned* list = lists + (size_t)slot * stride;
    for (int e = part * 256 + tid; e < total; e += kListParts * 256) {
        int a = 0, b = items;                                           // the last item whose offset is <= e: the one with a block number e
        while (b - a > 1) { const int m = (a + b) >> 1; if (off[m] <= e) a = m; else b = m; }
        int nb[3];
        blocks_of(a, nb);
        const int r = e - off[a], s = a / n;
        list[e] = wino_list_entry(a - s * n, s, r / (nb[2] * nb[1]), (r / nb[2]) % nb[1], r % nb[2]);
    }
}

// The XCD dealing of an own-cover launch.  Its grid is the LARGEST tile's, so a smaller tile's surplus workgroups return at once -- and xcd_block_id deals
// logical ids, not work: with the option's 32 ids per deal and, e.g., 8 ids per tile (dc8's y strip of the 160-tile volume) XCD k gets the tiles of ONE y
// row of the tile grid, four XCDs get every live block and four get none (kernel trace, profiles/own_cover.md: 2.22 ms, against 1.37 ms dealt 20 ids at a
// time; dc7's y strip 0.83 -> 0.51 ms).  The host knows
// every tile's live blocks (tile_nb: [tile] rows of kTileNbStride, this launch's three counts at the pointer), so it counts the live workgroups each XCD
// would get for a few granularities and takes the one with the lightest heaviest XCD -- the option's own unless another is at least 2 % better.  Neighbours
// in x and the cout blocks of one spatial block still share an L2 (>= 16 ids per deal).  Where a block runs does not change its bits.
static int balanced_xcd_group(int configured, const int* tile_nb, int ntiles, const int nb[3], int ncb) {
    if (configured <= 0) return configured;
    auto heaviest = [&](int G) {
        long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int t = 0; t < ntiles; ++t) {
            const int* tn = tile_nb + (size_t)t * kTileNbStride;
            for (int bz = 0; bz < tn[0]; ++bz)
                for (int by = 0; by < tn[1]; ++by) {                            // the live ids of one block row are consecutive: bx and the cout block run fastest
                    long long id = (((long long)t * nb[0] + bz) * nb[1] + by) * nb[2] * ncb, left = (long long)tn[2] * ncb;
                    while (left > 0) {
                        const long long g = id / G, take = std::min(left, (g + 1) * G - id);
                        load[g & 7] += take; id += take; left -= take;
                    }
                }
        }
        return *std::max_element(load, load + 8);
    };
    int best = configured;
    long long best_load = heaviest(configured);
    for (int G = 30; G >= 16 && best_load > 0; G -= 2) {
        const long long l = heaviest(G);
        if (l * 100 < best_load * 98) { best = G; best_load = l; }
    }
    return best;
}


// everything of ConvArgs that does not depend on the tile shape
int fill_conv_args(const oai_unet* h, const Layer& L, const float* s0, const float* s1, float* out, const int dims[3], const ConvOpt& o, ConvArgs& a) {
    if (o.head) a = *o.head;               // the fused dc0 fields (see ConvArgs); everything else is set below
    if (o.store_boxes && h->sres && h->opt_dead_stores) { a.store_boxes = o.store_boxes; a.store_grow = 1; }
    if (o.first) {                         // ec0 fused into this layer's staging (first_fusable)
        a.first_w = h->L[EC0].plain; a.first_scale = h->L[EC0].scale_f16; a.first_shift = h->L[EC0].shift_f16; a.first_src = *o.first;   // (sres => fp16x3)
        a.first_census = census_of(h, EC0);
    }
    if (const Scatter* sc = o.sc) {
        a.sc_boxes = sc->boxes; a.sc_ntiles = sc->ntiles; a.sc_tile0 = sc->tile0;
        for (int i = 0; i < 3; ++i) { a.sc_g[i] = sc->g[i]; a.sc_e[i] = sc->e[i]; a.sc_t[i] = sc->t[i]; }
    }
    a.boxes = o.boxes;
    a.pool_out = o.pool_out;
    a.range_flag = h->range_flag;
#ifdef OAI_DIAG
    a.stamps = layer_stamps(h, L);
#endif
    a.src0 = s0; a.src1 = s1; a.C0 = L.c0; a.C1 = s1 ? L.c1 : 0;
    const bool f16 = h->precision == OAI_PREC_FP16X3;
    a.out = out; a.Cout = L.cout; a.scale = f16 ? L.scale_f16 : L.scale; a.shift = f16 ? L.shift_f16 : L.shift;
    a.census = h->sres ? census_of(h, layer_id(h, L)) : nullptr;
    a.wpanel = h->precision == OAI_PREC_F32 ? L.panel : L.panel_bf[h->precision == OAI_PREC_BF16X3 ? 0 : h->precision == OAI_PREC_BF16X6 ? 1 : 2];
    a.wpanel16 = h->precision == OAI_PREC_FP16X3 && layer_bit(h, h->opt_m16_layers, L) ? L.panel_m16 : nullptr;
    a.D = dims[0]; a.H = dims[1]; a.W = dims[2];
    a.ncb = (L.cout + 63) / 64;
    a.relu = 1;
    if (h->sres && (size_t)dims[0] * dims[1] * dims[2] * 128 >= (1ull << 32))      // staging plan and copy-out hold 32-bit byte offsets inside one / two chunk planes
        return set_error(OAI_ERR_ARG, "tile level %dx%dx%d too large for the split-resident kernel (>= 2^25 voxels)", dims[0], dims[1], dims[2]);
    return OAI_OK;
}

// One k3 conv layer: fills its arguments and picks the kernel family that runs it -- Winograd in exact fp32 (unet_wino.hip), Winograd split-resident
// (the same file), or the direct kernels (unet_direct.hip), which take whatever the first two leave
static int launch_conv3(const oai_unet* h, const Layer& L, const float* s0, const float* s1, float* out,
                        const int dims[3], const Box& box, int ntiles, hipStream_t st, const ConvOpt& o = {}) {
    ConvArgs a;
    if (int rc = fill_conv_args(h, L, s0, s1, out, dims, o, a)) return rc;
    if (h->precision == OAI_PREC_F32 && h->variant == 0 && h->opt_wino_f32 && L.panel_wino_f32 && a.Cout % 4 == 0 && !a.head_w && !a.first_w && !a.sc_boxes &&
        (!a.pool_out || (wino_pool_box(box, dims) && dims[0] % 2 == 0)) && layer_bit(h, h->opt_wino_layers, L))
        return launch_conv3_wino_f32(h, L, a, box, ntiles, st);
    if (h->sres && h->opt_wino && L.panel_wino && h->sres_mrep == 4 && !a.first_w && !a.head_w && !a.sc_boxes &&
        (!a.pool_out || (a.Cout % 128 == 0 && a.relu && wino_pool_box(box, dims))) && a.Cout % 64 == 0 && (h->opt_wino & (a.Cout % 128 == 0 ? 1 : 2)) && (a.Cout % 128 == 0 || (a.C0 + 15) / 16 + (a.C1 + 15) / 16 >= 8) && layer_bit(h, h->opt_wino_layers, L) && (size_t)dims[0] * dims[1] * dims[2] < (1u << 24))
        return launch_conv3_wino(h, L, a, box, ntiles, st, o.oc);
    return launch_conv3_direct(h, a, box, ntiles, st);
}

// MaxPool3d(2) can ride in the conv epilogue when the (full) box is tiled exactly by the main 4 x 8 x 16 shape
static bool pool_fusable(const oai_unet* h, const int dims[3], const Box& box) {
    if (h->variant != 0) return false;
    for (int i = 0; i < 3; ++i) if (box.lo[i] != 0 || box.hi[i] != dims[i]) return false;
    return dims[0] % 4 == 0 && dims[1] % 8 == 0 && dims[2] % 16 == 0;
}

// Shared encoder pass.  Tiles overlap 2 x in z and 1.33 x in y and x, so ec0 / ec1 evaluate every input voxel ~3.6 x.  An ec1
// output at least 2 voxels from its tile's faces sees no zero padding (ec0 differs from the volume-wide convolution at distance 0, ec1 at
// distances 0 and 1) and -- every launch accumulates in the same k order -- is BIT-IDENTICAL in every tile that contains it.  So ec0 -> ec1
// (+ the fused max-pool) run ONCE per batch over the part of the reflect-padded volume its tiles cover, as one big "tile": the pooled tensor
// goes to SP0 (volume strides), and the copy-out of ec1 itself scatters every voxel straight into the per-tile syn0 tensors of the tiles
// whose dc2 reads it (the skip read [need - 1, need + 1) lies inside the interior).  Per tile only the 2-voxel shell of ec1 is recomputed
// (ec0 on a 3-voxel shell, six thin face launches, the pooled faces) and the interior of the tile's pooled tensor is copied out of SP0.
// ec1 is 22 ms of a 169 ms volume at 0.167 of the MFMA peak; the shared pass takes 8.7 ms.

// One batch of `n` tiles through the whole network; kept-centre blocks go to blocks_out.
// `table` (device, may be null) = per-tile boxes [layer][table_tiles][6] of the whole call; this batch starts at tile
// `t0` of it.  For up-convs the table row holds the INPUT box (the halved output box).
static int run_batch(oai_unet* h, const TileSource& src, int n, const Box need[18], int out_mode,
                     float* blocks_out, float* const buf[B_COUNT], hipStream_t st,
                     const int* table = nullptr, int table_tiles = 0, int t0 = 0, const SharedEnc* se = nullptr, const OwnPlan* own = nullptr) {
    auto tb = [&](int layer) -> const int* { return table ? table + ((size_t)layer * table_tiles + t0) * 6 : nullptr; };
    if (!table || !h->opt_own_cover) own = nullptr;
    OwnCover ocs[kOwnLayers];
    auto oc = [&](int layer) -> const OwnCover* {                     // the layer's own-cover rows and grids (option "own_cover"), or null
        if (!own) return nullptr;
        const int slot = own_cover_slot(layer);
        ocs[slot].list = own->list[slot]; ocs[slot].list_len = own->list_len[slot];      // option "one_launch": one launch over the live blocks -- nothing to balance
        for (int s = 0; s < 3; ++s) {
            ocs[slot].rows[s] = tb(18 + 3 * slot + s);
            for (int i = 0; i < 3; ++i) ocs[slot].nb[s][i] = own->nb[slot][s][i];
            // (counted here, just before the layer's launches: under the device work queued so far)
            const int ncb = h->L[layer].cout / (64 * wino_groups(h, h->L[layer].cout, kWinoTY[s]));
            ocs[slot].xcd_group[s] = own->nb[slot][s][0] && ncb > 0 && !ocs[slot].list_len ? balanced_xcd_group(h->xcd_group, own->tile_nb.data() + (slot * 3 + s) * 3, n, own->nb[slot][s], ncb) : 0;
        }
        return &ocs[slot];
    };
    auto upv = [&](int layer) { return own ? own->up_nvox[layer] : 0; };
    const Layer* L = h->L;
    int d[4][3];
    for (int l = 0; l < 4; ++l) { d[l][0] = src.td >> l; d[l][1] = src.th >> l; d[l][2] = src.tw >> l; }

    int rc;
#define RUN(x) do { rc = (x); if (rc) return rc; } while (0)
    if (se) {
        // ---- ec0 -> ec1 once over the z range of the padded volume that this batch's tiles cover
        {
            TileSource vs{};                                        // the padded volume as ONE tile: reflect_index(c - overlap) is Partition's padding
            vs.vol = se->vol; vs.D = se->D; vs.H = se->H; vs.W = se->W; vs.td = se->PD; vs.th = se->PH; vs.tw = se->PW;
            vs.ez = se->PD; vs.ey = se->PH; vs.ex = se->PW; vs.oz = se->overlap[0]; vs.oy = se->overlap[1]; vs.ox = se->overlap[2]; vs.gy = 1; vs.gx = 1;
            const int per_row = se->grid[1] * se->grid[2], P[3] = {se->PD, se->PH, se->PW};
            Scatter sc;
            sc.boxes = tb(DC2); sc.ntiles = n; sc.tile0 = src.tile_begin;
            for (int i = 0; i < 3; ++i) { sc.g[i] = se->grid[i]; sc.e[i] = se->eff[i]; }
            sc.t[0] = src.td; sc.t[1] = src.th; sc.t[2] = src.tw;
            // One launch per z slab of `eff` slices, over the y / x BOUNDING BOX of the batch's tiles that touch the slab (a tile of z row i
            // covers the slabs [i, i + td / eff)): a whole volume is one box per slab = the full y / x extent as before, but a rank's share of
            // a tile-sharded volume (19-23 tiles = parts of two or three z rows) no longer pays for the full extent of every row it touches
            // (round 4: profiles/r04_tileshard_projection.md).  Values do not depend on the box: the halo is read from the padded volume.
            const int t_first = src.tile_begin, t_last = src.tile_begin + n - 1;
            const int zspan = (src.td + se->eff[0] - 1) / se->eff[0];           // slabs per tile (2 for 32 / 16)
            const int s_first = t_first / per_row, s_last = t_last / per_row + zspan - 1;
            Box prev{}; bool have_prev = false;
            for (int s = s_first; s <= s_last; ++s) {
                int jlo = 1 << 30, jhi = -1, klo = 1 << 30, khi = -1;
                for (int i = s - zspan + 1; i <= s; ++i) {                      // z rows whose tiles cover slab s
                    if (i < 0 || i >= se->grid[0]) continue;
                    const int a0 = std::max(t_first, i * per_row), a1 = std::min(t_last, (i + 1) * per_row - 1);
                    if (a0 > a1) continue;
                    const int j0 = (a0 - i * per_row) / se->grid[2], j1 = (a1 - i * per_row) / se->grid[2];
                    jlo = std::min(jlo, j0); jhi = std::max(jhi, j1);
                    if (j0 == j1) { klo = std::min(klo, (a0 - i * per_row) % se->grid[2]); khi = std::max(khi, (a1 - i * per_row) % se->grid[2]); }
                    else { klo = 0; khi = se->grid[2] - 1; }
                }
                if (jhi < 0) continue;
                Box bx;
                bx.lo[0] = se->eff[0] * s; bx.hi[0] = std::min(P[0], se->eff[0] * (s + 1));
                if (s == s_last) bx.hi[0] = std::min(P[0], se->eff[0] * (t_last / per_row) + src.td);       // (the last slab takes the remainder of the tile height)
                bx.lo[1] = se->eff[1] * jlo; bx.hi[1] = std::min(P[1], se->eff[1] * jhi + src.th);
                bx.lo[2] = se->eff[2] * klo; bx.hi[2] = std::min(P[2], se->eff[2] * khi + src.tw);
                if (have_prev && prev.lo[1] == bx.lo[1] && prev.hi[1] == bx.hi[1] && prev.lo[2] == bx.lo[2] && prev.hi[2] == bx.hi[2] && prev.hi[0] == bx.lo[0]) {
                    prev.hi[0] = bx.hi[0];                                      // same footprint as the slab below: one launch for both
                    continue;
                }
                if (have_prev) RUN(launch_conv3(h, L[EC1], nullptr, nullptr, buf[B_SYN0], P, prev, 1, st, {.pool_out = se->SP0, .first = &vs, .sc = &sc}));
                prev = bx; have_prev = true;
            }
            if (have_prev) RUN(launch_conv3(h, L[EC1], nullptr, nullptr, buf[B_SYN0], P, prev, 1, st, {.pool_out = se->SP0, .first = &vs, .sc = &sc}));
        }
        // ---- the interior of this batch's pooled tensors is a copy, their faces are computed
        RUN(launch_pooled_gather(h, *se, src, buf[B_P0], d[1], n, st));
        RUN(launch_first_shell(h, src, buf[B_E0], d[0], n, st));        // ec0 where ec1's shell reads it
        const int td = d[0][0], th = d[0][1], tw = d[0][2];
        const Box zlo = {{0, 0, 0}, {2, th, tw}}, zhi = {{td - 2, 0, 0}, {td, th, tw}};                      // the six faces, 2 voxels thick, disjoint
        const Box ylo = {{2, 0, 0}, {td - 2, 2, tw}}, yhi = {{2, th - 2, 0}, {td - 2, th, tw}};
        const Box xlo = {{2, 2, 0}, {td - 2, th - 2, 2}}, xhi = {{2, 2, tw - 2}, {td - 2, th - 2, tw}};
        // z faces: main shape with 2 slices per block; nobody reads their part of the per-tile syn0, only its max-pool (fused into the launch)
        const bool zpool = tb(EC1) != nullptr && h->opt_dead_stores;
        RUN((launch_conv3_one<16, 2, 4, 1>(h, L[EC1], buf[B_E0], buf[B_SYN0], d[0], zlo, n, st, tb(EC1), zpool ? buf[B_P0] : nullptr)));
        RUN((launch_conv3_one<16, 2, 4, 1>(h, L[EC1], buf[B_E0], buf[B_SYN0], d[0], zhi, n, st, tb(EC1), zpool ? buf[B_P0] : nullptr)));
        RUN((launch_conv3_one<16, 2, 1, 4>(h, L[EC1], buf[B_E0], buf[B_SYN0], d[0], ylo, n, st, tb(EC1))));   // y faces: blocks of 4 x 2 x 64
        RUN((launch_conv3_one<16, 2, 1, 4>(h, L[EC1], buf[B_E0], buf[B_SYN0], d[0], yhi, n, st, tb(EC1))));
        RUN((launch_conv3_one<2, 16, 4, 1>(h, L[EC1], buf[B_E0], buf[B_SYN0], d[0], xlo, n, st, tb(EC1))));   // x faces: blocks of 4 x 64 x 2
        RUN((launch_conv3_one<2, 16, 4, 1>(h, L[EC1], buf[B_E0], buf[B_SYN0], d[0], xhi, n, st, tb(EC1))));
        RUN(launch_pool(h, buf[B_SYN0], buf[B_P0], d[0], L[EC1].cout, n, st, zpool ? 2 : 1));               // the (other) pooled faces: windows inside the shell
    } else {
    const bool fuse_first = first_fusable(h, need[EC1]);
    const TileSource* fsrc = fuse_first ? &src : nullptr;
    if (!fuse_first) RUN(launch_first(h, src, buf[B_E0], n, st));   // ec0 (+ gather)
    if (pool_fusable(h, d[0], need[EC1])) {
        RUN(launch_conv3(h, L[EC1], buf[B_E0], nullptr, buf[B_SYN0], d[0], need[EC1], n, st, {.boxes = tb(EC1), .pool_out = buf[B_P0], .first = fsrc, .store_boxes = tb(DC2)}));
    } else {
        RUN(launch_conv3(h, L[EC1], buf[B_E0], nullptr, buf[B_SYN0], d[0], need[EC1], n, st, {.boxes = tb(EC1), .first = fsrc}));
        RUN(launch_pool(h, buf[B_SYN0], buf[B_P0], d[0], L[EC1].cout, n, st));
    }
    }
    RUN(launch_conv3(h, L[EC2], buf[B_P0], nullptr, buf[B_E2], d[1], need[EC2], n, st, {.boxes = tb(EC2)}));
    if (pool_fusable(h, d[1], need[EC3])) {
        RUN(launch_conv3(h, L[EC3], buf[B_E2], nullptr, buf[B_SYN1], d[1], need[EC3], n, st, {.boxes = tb(EC3), .pool_out = buf[B_P1], .store_boxes = tb(DC5)}));
    } else {
        RUN(launch_conv3(h, L[EC3], buf[B_E2], nullptr, buf[B_SYN1], d[1], need[EC3], n, st, {.boxes = tb(EC3)}));
        RUN(launch_pool(h, buf[B_SYN1], buf[B_P1], d[1], L[EC3].cout, n, st));
    }
    RUN(launch_conv3(h, L[EC4], buf[B_P1], nullptr, buf[B_E4], d[2], need[EC4], n, st, {.boxes = tb(EC4)}));
    if (pool_fusable(h, d[2], need[EC5])) {
        RUN(launch_conv3(h, L[EC5], buf[B_E4], nullptr, buf[B_SYN2], d[2], need[EC5], n, st, {.boxes = tb(EC5), .pool_out = buf[B_P2], .store_boxes = tb(DC8)}));
    } else {
        RUN(launch_conv3(h, L[EC5], buf[B_E4], nullptr, buf[B_SYN2], d[2], need[EC5], n, st, {.boxes = tb(EC5)}));
        RUN(launch_pool(h, buf[B_SYN2], buf[B_P2], d[2], L[EC5].cout, n, st));
    }
    RUN(launch_conv3(h, L[EC6], buf[B_P2], nullptr, buf[B_E6], d[3], need[EC6], n, st, {.boxes = tb(EC6)}));
    RUN(launch_conv3(h, L[EC7], buf[B_E6], nullptr, buf[B_E7], d[3], need[EC7], n, st, {.boxes = tb(EC7)}));
    RUN(launch_up(h, L[DC9], buf[B_E7], buf[B_U9], d[3], need[DC9], n, st, tb(DC9), upv(DC9)));
    RUN(launch_conv3(h, L[DC8], buf[B_U9], buf[B_SYN2], buf[B_D8], d[2], need[DC8], n, st, {.boxes = tb(DC8), .oc = oc(DC8)}));   // cat(up, skip) :127
    RUN(launch_conv3(h, L[DC7], buf[B_D8], nullptr, buf[B_D7], d[2], need[DC7], n, st, {.boxes = tb(DC7), .oc = oc(DC7)}));
    RUN(launch_up(h, L[DC6], buf[B_D7], buf[B_U6], d[2], need[DC6], n, st, tb(DC6), upv(DC6)));
    RUN(launch_conv3(h, L[DC5], buf[B_U6], buf[B_SYN1], buf[B_D5], d[1], need[DC5], n, st, {.boxes = tb(DC5), .oc = oc(DC5)}));   // :134
    RUN(launch_conv3(h, L[DC4], buf[B_D5], nullptr, buf[B_D4], d[1], need[DC4], n, st, {.boxes = tb(DC4), .oc = oc(DC4)}));
    RUN(launch_up(h, L[DC3], buf[B_D4], buf[B_U3], d[1], need[DC3], n, st, tb(DC3), upv(DC3)));
    RUN(launch_conv3(h, L[DC2], buf[B_U3], buf[B_SYN0], buf[B_D2], d[0], need[DC2], n, st, {.boxes = tb(DC2), .oc = oc(DC2)}));   // :141
    // dc0 + sigmoid/threshold + centre crop: blocks are laid out over the full kept centre.  In the split-resident path it rides
    // in dc1's epilogue (dc1's 64 output channels sit in one workgroup): no dc1 output round trip through HBM, no head launch.
    const int hk[3] = {src.vol ? src.oz : 0, src.vol ? src.oy : 0, src.vol ? src.ox : 0};
    const int he[3] = {src.vol ? src.ez : src.td, src.vol ? src.ey : src.th, src.vol ? src.ex : src.tw};
    static const bool no_fuse = diag_env("OAI_NO_HEAD_FUSE", 0) != 0;
    const bool fuse_head = h->sres && !no_fuse && L[DC1].cout <= 64 && L[DC0].cin == L[DC1].cout && h->n_classes <= 4 &&
                           need[DC1].lo[0] <= need[DC0].lo[0] && need[DC1].hi[0] >= need[DC0].hi[0];
    if (fuse_head) {
        ConvArgs ha;
        ha.head_w = L[DC0].plain_f16; ha.head_b = L[DC0].shift;       // (fuse_head => sres => fp16x3: head weights carry 2^-e(dc1))
        ha.head_boxes = tb(DC0); ha.head_out = blocks_out;
        ha.head_ncls = h->n_classes; ha.head_mode = out_mode;
        for (int i = 0; i < 3; ++i) { ha.head_k[i] = hk[i]; ha.head_e[i] = he[i]; }
        RUN(launch_conv3(h, L[DC1], buf[B_D2], nullptr, buf[B_D1], d[0], need[DC0], n, st, {.boxes = tb(DC0), .head = &ha}));
        return OAI_OK;
    }
    RUN(launch_conv3(h, L[DC1], buf[B_D2], nullptr, buf[B_D1], d[0], need[DC1], n, st, {.boxes = tb(DC1)}));
    RUN(launch_head(h, buf[B_D1], d[0], need[DC0], hk, he, out_mode, blocks_out, tb(DC0), n, st));
#undef RUN
    return OAI_OK;
}

static double layer_flops(const oai_unet* h, int k, const Box& b) {
    const double vox = (double)(b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]);
    const int taps = (layer_kind(k) == 0 || layer_kind(k) == 1) ? 27 : 1;
    return 2.0 * vox * taps * h->L[k].cin * h->L[k].cout;
}

constexpr int kTargetExp = 10;            // calibration puts a layer's maximum in [2^10, 2^11)

}  // namespace oai

using namespace oai;

// one zero-filled device block of the handle (freed by oai_unet_destroy)
template <typename T>
static int alloc_zeroed(oai_unet* h, size_t bytes, T** ptr) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) return set_error(OAI_ERR_HIP, "oai_unet_create: hipMalloc failed");
    h->allocs.push_back(d);
    (void)hipMemset(d, 0, bytes);
    *ptr = reinterpret_cast<T*>(d);
    return OAI_OK;
}

// k3 layers that run the implicit-GEMM conv kernels (ec0 and the 1x1x1 head have kernels of their own)
static inline bool is_conv3_igemm(int k) { return k >= 1 && k < 17 && (layer_kind(k) == 0 || layer_kind(k) == 1); }

static double tile_flops(const oai_unet* h, int td, int th, int tw, const int overlap[3], int trimmed, bool conv3_only) {
    if (!h) return 0.0;
    const int tile[3] = {td, th, tw};
    int lo[3], hi[3];
    for (int i = 0; i < 3; ++i) { lo[i] = overlap ? overlap[i] : 0; hi[i] = tile[i] - lo[i]; }
    Box need[18];
    plan_regions(tile, lo, hi, trimmed != 0, need);
    double f = 0;
    for (int k = 0; k < 18; ++k)
        if (!conv3_only || is_conv3_igemm(k)) f += layer_flops(h, k, need[k]);
    return f;
}

extern "C" {

int oai_unet_create(const oai_layer_params layers[OAI_UNET_NUM_LAYERS], float bn_eps, oai_unet** out) {
    OAI_CHECK_ARG(layers && out, "oai_unet_create: null pointer");
    for (int k = 0; k < 18; ++k) {
        OAI_CHECK_ARG(layers[k].weight_host, "oai_unet_create: layer %d has no weight (strict load)", k);
        OAI_CHECK_ARG(layers[k].kind == layer_kind(k), "oai_unet_create: layer %d kind %d, expected %d", k, layers[k].kind, layer_kind(k));
        OAI_CHECK_ARG(layers[k].cin > 0 && layers[k].cout > 0, "oai_unet_create: layer %d bad channels", k);
    }
    // channel wiring of UNet.__init__ (networks.py:43-66)
    const int chain[][2] = {{EC0, EC1}, {EC1, EC2}, {EC2, EC3}, {EC3, EC4}, {EC4, EC5}, {EC5, EC6}, {EC6, EC7}, {EC7, DC9},
                            {DC8, DC7}, {DC7, DC6}, {DC5, DC4}, {DC4, DC3}, {DC2, DC1}, {DC1, DC0}};
    for (auto& c : chain)
        OAI_CHECK_ARG(layers[c[0]].cout == layers[c[1]].cin, "oai_unet_create: layer %d cout != layer %d cin", c[0], c[1]);
    OAI_CHECK_ARG(layers[DC8].cin == layers[DC9].cout + layers[EC5].cout, "oai_unet_create: dc8 cin != dc9 + ec5");
    OAI_CHECK_ARG(layers[DC5].cin == layers[DC6].cout + layers[EC3].cout, "oai_unet_create: dc5 cin != dc6 + ec3");
    OAI_CHECK_ARG(layers[DC2].cin == layers[DC3].cout + layers[EC1].cout, "oai_unet_create: dc2 cin != dc3 + ec1");
    OAI_CHECK_ARG(layers[EC0].cin == 1, "oai_unet_create: only in_channels == 1 is supported (the reference's config)");
    OAI_CHECK_ARG(layers[DC0].cout <= 4, "oai_unet_create: n_classes must be <= 4");
    for (int k = 0; k < 18; ++k) {
        OAI_CHECK_ARG(k == EC0 || layers[k].cin % 8 == 0, "oai_unet_create: layer %d cin must be a multiple of 8", k);
        OAI_CHECK_ARG(k == DC0 || layers[k].cout % 8 == 0, "oai_unet_create: layer %d cout must be a multiple of 8", k);
    }

    oai_unet* h = new oai_unet();
    int rc = alloc_zeroed(h, 256, &h->range_flag);
    if (!rc) rc = alloc_zeroed(h, 256, &h->zero_rec);
    if (!rc) rc = alloc_zeroed(h, 18 * 16 * sizeof(unsigned) + 256, &h->census);      // the census, then the scratch word of oai_unet_range_flag
    if (rc) { oai_unet_destroy(h); return rc; }
    h->eval_out = reinterpret_cast<int*>(h->census + 18 * 16);
    h->variant = diag_env("OAI_CONV_VARIANT", 0);
    if (h->variant < 0 || h->variant > 2) h->variant = 0;
    h->n_classes = layers[DC0].cout;
    const int KC = conv_kc(h->variant);
    for (int k = 0; k < 18 && rc == OAI_OK; ++k) {
        const oai_layer_params& p = layers[k];
        Layer& L = h->L[k];
        L.kind = p.kind; L.cin = p.cin; L.cout = p.cout; L.c0 = p.cin; L.c1 = 0;
        if (k == DC8) { L.c0 = layers[DC9].cout; L.c1 = layers[EC5].cout; }
        if (k == DC5) { L.c0 = layers[DC6].cout; L.c1 = layers[EC3].cout; }
        if (k == DC2) { L.c0 = layers[DC3].cout; L.c1 = layers[EC1].cout; }
        // epilogue affine: eval-mode BatchNorm3d folded with the conv bias (per channel, weights untouched)
        std::vector<float> sc(p.cout, 1.0f), sh(p.cout, 0.0f);
        for (int c = 0; c < p.cout; ++c) {
            const float b = p.bias_host ? p.bias_host[c] : 0.0f;
            if (p.bn_gamma_host) {
                const float s = p.bn_gamma_host[c] / sqrtf(p.bn_var_host[c] + bn_eps);
                sc[c] = s;
                sh[c] = (b - p.bn_mean_host[c]) * s + p.bn_beta_host[c];
            } else sh[c] = b;
        }
        L.scale_host = sc; L.shift_host = sh;
        if ((rc = upload(h, sc, &L.scale))) break;
        if ((rc = upload(h, sh, &L.shift))) break;
        if (k == EC0) {
            std::vector<float> wk = canonical_k3(p);          // [27][1][cout]
            rc = upload(h, wk, &L.plain);
        } else if (p.kind == 0 || p.kind == 1) {
            L.wk_host = canonical_k3(p);
            rc = upload(h, pack_conv3_panel(L.wk_host, L.c0, L.c1, p.cout, KC), &L.panel);
            if (!rc && KC == 8) rc = upload(h, pack_wino_f32_panel(L.wk_host, L.c0, L.c1, p.cout), &L.panel_wino_f32);
        } else if (p.kind == 2) {
            L.wk_host.assign(p.weight_host, p.weight_host + (size_t)p.cin * p.cout * 8);     // [ci][co][2][2][2], for re-packing
            rc = upload(h, pack_up_panel(p), &L.panel);
        } else {
            std::vector<float> w(p.weight_host, p.weight_host + (size_t)p.cout * p.cin);
            L.plain_host = w;
            rc = upload(h, w, &L.plain);
        }
    }
    if (rc != OAI_OK) { oai_unet_destroy(h); return rc; }
    *out = h;
    return OAI_OK;
}

int oai_unet_set_precision(oai_unet* h, int mode) {
    OAI_CHECK_ARG(h, "oai_unet_set_precision: null handle");
    OAI_CHECK_ARG(mode >= OAI_PREC_F32 && mode <= OAI_PREC_FP16X3, "oai_unet_set_precision: unknown mode %d", mode);
    OAI_CHECK_ARG(mode == OAI_PREC_F32 || h->variant == 0, "oai_unet_set_precision: split modes need OAI_CONV_VARIANT=0");
    if (mode != OAI_PREC_F32) {
        const int slot = mode == OAI_PREC_BF16X3 ? 0 : mode == OAI_PREC_BF16X6 ? 1 : 2, NS = slot == 1 ? 3 : 2;
        for (int k = 1; k < 17; ++k) {
            Layer& L = h->L[k];
            if (slot == 2) {                                           // fp16x3: k3 convs and k2s2 up-convs (pack_fp16_layer)
                if (!L.panel_bf[2])
                    if (int rc = pack_fp16_layer(h, k)) return rc;
                continue;
            }
            if ((L.kind != 0 && L.kind != 1) || L.panel_bf[slot]) continue;
            if (int rc = upload(h, pack_conv3_panel_bf(L.wk_host, L.c0, L.c1, L.cout, NS), &L.panel_bf[slot])) return rc;
        }
        if (slot == 2 && !h->L[EC0].scale_f16)
            if (int rc = refresh_fp16_affine(h)) return rc;
    }
    h->precision = mode;
    h->sres = mode == OAI_PREC_FP16X3 && h->opt_sres;
    return OAI_OK;
}

// The options that are one int in a range, one row each: name, field, lo, hi, the message for a value outside [lo, hi] -- and what the option does.
struct IntOption { const char* name; int oai_unet::*field; int lo, hi; const char* message; };
static const IntOption kIntOptions[] = {
    // ec0 -> ec1 computed ONCE over the reflect-padded volume + a 2-voxel shell per tile (oai_segment_tiles)
    {"shared_enc", &oai_unet::opt_shared, 0, 1, "oai_unet_set_option: shared_enc must be 0 or 1"},
    // layers with Cout % 128 == 0 run conv3_igemm_sres2 (one 8-wave workgroup per CU, double-buffered halo)
    {"wide", &oai_unet::opt_wide, 0, 2, "oai_unet_set_option: wide must be 0, 1 or 2 (2 = also for launches of fewer than 1024 workgroups)"},
    // bit k = layer k may take the Winograd kernel (A/B of single layers)
    {"winograd_layers", &oai_unet::opt_wino_layers, 0, 0x3FFFF, "oai_unet_set_option: winograd_layers is a mask over the 18 layers"},
    // the direct split-resident kernel (conv3_igemm_sres: ec1 + fused ec0, ec2, dc1 + fused head, ...) on v_mfma_f32_16x16x32_f16 tap pairs (round 5; another
    // summation order; default 1) for every layer that can never take the bit-identical 128-cout form conv3_igemm_sres2 -- i.e. Cout % 128 != 0 -- so that a
    // layer runs ONE order whatever shapes cover it and option "wide" stays bit-preserving
    {"m16", &oai_unet::opt_m16, 0, 1, "oai_unet_set_option: m16 must be 0 or 1"},
    // bit k = layer k may take the tap-pair form (A/B of single layers)
    {"m16_layers", &oai_unet::opt_m16_layers, 0, 0x3FFFF, "oai_unet_set_option: m16_layers is a mask over the 18 layers"},
    // 1 = the encoder does not write the part of a skip tensor that the decoder never reads
    {"dead_stores", &oai_unet::opt_dead_stores, 0, 1, "oai_unet_set_option: dead_stores must be 0 or 1"},
    // NOT bit-preserving: the plain k3 layers of the exact-fp32 path run conv3_wino_f32 (x axis in Winograd F(2,3) form: 2/3 of the fp32 MFMAs)
    {"winograd_f32", &oai_unet::opt_wino_f32, 0, 1, "oai_unet_set_option: winograd_f32 must be 0 or 1"},
    // bit-preserving: workgroups per tile of the ec0 kernel conv3_first_sres_kernel (each walks the tile's voxel pairs with a grid stride, the next pair's
    // gathers under the current pair's FMAs)
    {"first_blocks", &oai_unet::opt_first_blocks, 1, 4096, "oai_unet_set_option: first_blocks must be in [1, 4096]"},
    // bit-preserving: column blocks per workgroup of the k2s2 up-conv kernel: 0 = as many as keep >= 16 workgroups per slot, 1 = one (rounds 1-5), n = at most n
    {"up_nbw", &oai_unet::opt_up_nbw, 0, 64, "oai_unet_set_option: up_nbw must be in [0, 64]"},
    // bit-preserving: in oai_segment_tiles the trimmed decoder convs (dc8, dc7, dc5, dc4, dc2 on conv3_wino_sres) place their blocks on every tile's own cover
    // (tile_cover) and the up-convs list every tile's own input voxels, instead of the cover / the voxels of the batch's union box; 0 = the union's (A/B)
    {"own_cover", &oai_unet::opt_own_cover, 0, 1, "oai_unet_set_option: own_cover must be 0 or 1"},
    // bit-preserving: an own-cover layer runs as ONE launch over the batch's live-block list (conv3_wino_list*, unet_wino.h) instead of one launch per block
    // shape.  bit 0: the two-group layers (dc8, dc7, dc5, dc4), bit 1: the 64-cout layer (dc2), bit 2: also for a layer with fewer live blocks in the batch than
    // the device has CUs (one_launch_len: small batches keep their three launches unless a test forces it); 0 = three launches
    {"one_launch", &oai_unet::opt_one_launch, 0, 7, "oai_unet_set_option: one_launch must be in [0, 7] (bit 0 two-group layers, bit 1 the 64-cout layer, bit 2 force)"},
    // ec0 computed inside ec1's halo staging when ec1 is one main-shape launch
    {"fuse_first", &oai_unet::fuse_first, 0, 1, "oai_unet_set_option: fuse_first must be 0 or 1"},
    // logical blocks per XCD deal; 0 = plain launch order
    {"xcd_group", &oai_unet::xcd_group, 0, 4096, "oai_unet_set_option: xcd_group must be in [0, 4096]"},
};

// Result-preserving tuning options of the fp16x3 path (every combination is parity-tested: tests/test_unet_gpu.py).  An explicit
// call on the handle -- the production library does not read the environment.
int oai_unet_set_option(oai_unet* h, const char* name, int value) {
    OAI_CHECK_ARG(h && name, "oai_unet_set_option: null pointer");
    for (const IntOption& o : kIntOptions)
        if (!strcmp(name, o.name)) {
            OAI_CHECK_ARG(value >= o.lo && value <= o.hi, "%s", o.message);
            h->*o.field = value;
            return OAI_OK;
        }
    // the options with side effects or cross-checks
    if (!strcmp(name, "sres")) {                       // 1: activations resident as fp16 term pairs (default); 0: fp32-resident split kernels
        OAI_CHECK_ARG(value == 0 || value == 1, "oai_unet_set_option: sres must be 0 or 1");
        h->opt_sres = value != 0;
        h->sres = h->precision == OAI_PREC_FP16X3 && h->opt_sres;
    } else if (!strcmp(name, "sres_mrep")) {           // z slices per block of the split-resident conv kernel (2 runs three workgroups per CU: -2 % on 32 border tiles, +0.5 % on the whole volume)
        OAI_CHECK_ARG(value == 2 || value == 4, "oai_unet_set_option: sres_mrep must be 2 or 4");
        h->sres_mrep = value;
    } else if (!strcmp(name, "winograd")) {
        // plain k3 layers with Cout % 64 == 0 run conv3_wino_sres (x axis in Winograd F(2,3) form: 2/3 of the MFMAs).  bit 0: layers with Cout % 128 == 0 (two cout
        // groups per workgroup), bit 1: one block of 64 couts and >= 8 chunks (specialised waves); A/B only: bit 2 = the slice-split form instead, bit 3 = the
        // specialised form for every layer; bit 4 (round 4): the taps of the two-group form on v_mfma_f32_16x16x32_f16 (tap pairs: another summation order; same
        // cycles per FLOP, +14 % clock at the power wall); bit 5: the same for the 64-cout layer (dc2) -- ALL its launch shapes (specialised main blocks and x strip,
        // slice-split y strip: wino_m16_64), so a voxel's bits do not depend on the shape that covers it; measured within noise of bit 4 alone (-0.2 %), not the default
        OAI_CHECK_ARG(value >= 0 && value <= 63, "oai_unet_set_option: winograd must be in [0, 63]");
        if (value && !h->opt_wino && h->L[EC0].scale_f16) {
            OAI_CHECK_HIP(hipDeviceSynchronize());
            for (int k = 1; k < 17; ++k)
                if (h->L[k].panel_bf[2] && !h->L[k].panel_wino)
                    if (int rc = pack_wino_layer(h, k)) return rc;
        }
        h->opt_wino = value;
    } else if (!strcmp(name, "census")) {              // 0 = the kernels do not record the per-layer maxima (A/B timing of the bookkeeping; no LOW flag)
        OAI_CHECK_ARG(value == 0 || value == 1, "oai_unet_set_option: census must be 0 or 1");
        // without the census there is no LOW bit in the range flag and nothing to calibrate from: allowed on a calibrated handle only
        // (A/B timing of the bookkeeping), so that the subnormal low-term loss cannot come back silently
        OAI_CHECK_ARG(value == 1 || h->calibrated, "oai_unet_set_option: census 0 needs a calibrated handle (activation exponents set)");
        h->opt_census = value;
    } else if (!strcmp(name, "calibrated")) {          // only clearing: setting goes through oai_unet_set_act_exponents / a settled oai_unet_calibrate_step
        OAI_CHECK_ARG(value == 0, "oai_unet_set_option: calibrated can only be cleared (0)");
        OAI_CHECK_ARG(h->opt_census == 1, "oai_unet_set_option: an uncalibrated handle needs the census (option census is 0)");
        h->calibrated = false;
    } else {
        return set_error(OAI_ERR_ARG, "oai_unet_set_option: unknown option '%s'", name);
    }
    return OAI_OK;
}

int oai_unet_range_flag(oai_unet* h, int reset, int* out, void* stream) {
    OAI_CHECK_ARG(h && out, "oai_unet_range_flag: null pointer");
    // ordered on the caller's stream (the one the segment calls were queued on): torch's side streams are non-blocking, so
    // the null stream would not wait for them and a flag could be read -- and reset -- before the kernels that set it ran
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_range_eval(h, h->eval_out, reset, st)) return rc;
    OAI_CHECK_HIP(hipMemcpyAsync(out, h->eval_out, sizeof(int), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    return OAI_OK;
}

int oai_unet_range_flag_snapshot(oai_unet* h, int* dst_dev, void* stream) {
    OAI_CHECK_ARG(h && dst_dev, "oai_unet_range_flag_snapshot: null pointer");
    return launch_range_eval(h, dst_dev, 1, (hipStream_t)stream);   // a kernel: stream-ordered with the conv launches around it
}

int oai_unet_range_state_snapshot(oai_unet* h, int* state_dev, void* stream) {
    OAI_CHECK_ARG(h && state_dev, "oai_unet_range_state_snapshot: null pointer");
    return launch_range_state(h, state_dev, (hipStream_t)stream);
}

int oai_unet_range_flag_from_state(const int* state_dev, int* flag_dev, void* stream) {
    OAI_CHECK_ARG(state_dev && flag_dev, "oai_unet_range_flag_from_state: null pointer");
    return launch_range_flag_from_state(state_dev, flag_dev, (hipStream_t)stream);
}

int oai_unet_census(oai_unet* h, float max_out[OAI_UNET_NUM_LAYERS], int reset, void* stream) {
    OAI_CHECK_ARG(h && max_out, "oai_unet_census: null pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned host[18 * 16];
    OAI_CHECK_HIP(hipMemcpyAsync(host, h->census, sizeof(host), hipMemcpyDeviceToHost, st));
    OAI_CHECK_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 18; ++k) {
        unsigned m = 0;
        for (int i = 0; i < 16; ++i) m = host[k * 16 + i] > m ? host[k * 16 + i] : m;
        memcpy(&max_out[k], &m, 4);
    }
    if (reset) {
        OAI_CHECK_HIP(hipMemsetAsync(h->census, 0, sizeof(host), st));
        OAI_CHECK_HIP(hipMemsetAsync(h->range_flag, 0, sizeof(int), st));
    }
    return OAI_OK;
}

int oai_unet_get_act_exponents(const oai_unet* h, int e_out[OAI_UNET_NUM_LAYERS], int* calibrated) {
    OAI_CHECK_ARG(h && e_out, "oai_unet_get_act_exponents: null pointer");
    for (int k = 0; k < 18; ++k) e_out[k] = h->act_exp[k];
    if (calibrated) *calibrated = h->calibrated ? 1 : 0;
    return OAI_OK;
}

int oai_unet_set_act_exponents(oai_unet* h, const int e[OAI_UNET_NUM_LAYERS]) {
    OAI_CHECK_ARG(h && e, "oai_unet_set_act_exponents: null pointer");
    for (int k = 0; k < 17; ++k) OAI_CHECK_ARG(e[k] >= -100 && e[k] <= 100, "oai_unet_set_act_exponents: exponent %d of layer %d outside [-100, 100]", e[k], k);
    OAI_CHECK_ARG(e[DC0] == 0, "oai_unet_set_act_exponents: dc0 produces logits, its exponent must be 0");
    OAI_CHECK_HIP(hipDeviceSynchronize());               // the arrays rewritten below may be in use by queued launches (rare call: once per network)
    for (int k = 0; k < 18; ++k) h->act_exp[k] = e[k];
    h->calibrated = true;
    if (!h->L[EC0].scale_f16) return OAI_OK;             // fp16x3 not set up yet: oai_unet_set_precision packs with these exponents
    for (int k : {DC8, DC5, DC2}) {                      // concat layers: the panel carries 2^(e(src0) - e(src1)) on the skip channels
        const int rel1 = h->act_exp[layer_src0(k)] - h->act_exp[layer_src1(k)];
        if (rel1 != h->L[k].rel1)
            if (int rc = pack_fp16_layer(h, k)) return rc;
    }
    return refresh_fp16_affine(h);
}

int oai_unet_calibrate_step(oai_unet* h, void* stream, int* more) {
    OAI_CHECK_ARG(h && more, "oai_unet_calibrate_step: null pointer");
    OAI_CHECK_ARG(h->precision == OAI_PREC_FP16X3, "oai_unet_calibrate_step: the activation exponents belong to OAI_PREC_FP16X3");
    float mx[18];
    if (int rc = oai_unet_census(h, mx, 1, stream)) return rc;
    int e[18], changed = 0, reported = 0;
    for (int k = 0; k < 18; ++k) e[k] = h->act_exp[k];
    for (int k = 0; k < 17; ++k) {
        if (!(mx[k] > 0.0f)) continue;                   // nothing stored (layer not run by the split-resident kernels, or all zero): keep
        ++reported;
        if (!std::isfinite(mx[k])) { e[k] = e[k] - 32 < -100 ? -100 : e[k] - 32; changed = 1; continue; }
        int b;
        frexpf(mx[k], &b);                               // mx = m 2^b, m in [0.5, 1): mx in [2^(b-1), 2^b)
        if (b - 1 >= kTargetExp - 1 && b - 1 <= kTargetExp + 1) continue;       // inside [2^9, 2^12): leave it (a verify pass ends here)
        e[k] += kTargetExp - (b - 1);
        if (e[k] > 100) e[k] = 100;
        if (e[k] < -100) e[k] = -100;
        changed = 1;
    }
    *more = changed;
    // a census that holds nothing (option census 0 / sres 0 before the first run, or no pass queued since the last step) says
    // nothing about the exponents: refuse instead of reporting "calibrated" with whatever they were
    if (!reported)
        return oai::set_error(OAI_ERR_ARG, "oai_unet_calibrate_step: the range census is empty (no fp16x3 pass since the last step, or option census / sres is 0)");
    if (!changed) { h->calibrated = true; return OAI_OK; }
    const bool was = h->calibrated;
    const int rc = oai_unet_set_act_exponents(h, e);
    h->calibrated = was;                                 // exponents moved: only a later pass that finds every layer inside the window calibrates
    return rc;
}

int oai_unet_profile(oai_unet* h, int enable) {
    OAI_CHECK_ARG(h, "oai_unet_profile: null handle");
    h->profile = enable != 0;
    return OAI_OK;
}

int oai_unet_profile_read(oai_unet* h, double* conv3_ms, long long* conv3_launches) {
    OAI_CHECK_ARG(h && conv3_ms && conv3_launches, "oai_unet_profile_read: null pointer");
    double ms = 0.0;
    for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
        OAI_CHECK_HIP(hipEventSynchronize(h->ev_pool[i + 1]));
        float t = 0.0f;
        OAI_CHECK_HIP(hipEventElapsedTime(&t, h->ev_pool[i], h->ev_pool[i + 1]));
        ms += t;
    }
    *conv3_ms = ms;
    *conv3_launches = (long long)(h->ev_used / 2);
    h->ev_used = 0;
    return OAI_OK;
}

double oai_unet_tile_flops_conv3(const oai_unet* h, int td, int th, int tw, const int overlap[3], int trimmed) {
    return tile_flops(h, td, th, tw, overlap, trimmed, true);
}

void oai_unet_destroy(oai_unet* h) {
    if (!h) return;
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (void* p : h->allocs) (void)hipFree(p);
    delete h;
}

size_t oai_unet_workspace_bytes(const oai_unet* h, int td, int th, int tw, int batch) {
    if (!h || td <= 0 || th <= 0 || tw <= 0 || batch <= 0) return 0;
    return workspace_bytes(h, td, th, tw, batch);
}

double oai_unet_tile_flops(const oai_unet* h, int td, int th, int tw, const int overlap[3], int trimmed) {
    return tile_flops(h, td, th, tw, overlap, trimmed, false);
}

static int check_tile(int td, int th, int tw) {
    OAI_CHECK_ARG(td >= 8 && th >= 8 && tw >= 8 && td % 8 == 0 && th % 8 == 0 && tw % 8 == 0,
                  "tile size %dx%dx%d must be a positive multiple of 8 per axis (three 2x poolings)", td, th, tw);
    return OAI_OK;
}

int oai_unet_forward_tiles(oai_unet* h, const float* tiles, float* logits, int B, int td, int th, int tw,
                           void* ws, size_t ws_bytes, void* stream) {
    OAI_CHECK_ARG(h && tiles && logits && ws, "oai_unet_forward_tiles: null pointer");
    OAI_CHECK_ARG(B > 0, "oai_unet_forward_tiles: B must be > 0");
    if (int rc = check_tile(td, th, tw)) return rc;
    // as many tiles per pass as the workspace holds
    int batch = B;
    while (batch > 1 && workspace_bytes(h, td, th, tw, batch) > ws_bytes) --batch;
    float* buf[B_COUNT];
    int* table;
    const size_t need_bytes = carve_workspace(h, td, th, tw, batch, ws, buf, table);
    if (need_bytes > ws_bytes)
        return set_error(OAI_ERR_WORKSPACE, "oai_unet_forward_tiles: workspace %zu B < %zu B needed for one tile", ws_bytes, need_bytes);
    const int tile[3] = {td, th, tw};
    const int lo[3] = {0, 0, 0};
    Box need[18];
    plan_regions(tile, lo, tile, false, need);
    TileSource src{};
    src.vol = nullptr; src.td = td; src.th = th; src.tw = tw;
    const size_t v0 = (size_t)td * th * tw;
    for (int s = 0; s < B; s += batch) {
        const int n = B - s < batch ? B - s : batch;
        src.tiles = tiles + (size_t)s * v0;
        src.tile_begin = 0;
        if (int rc = run_batch(h, src, n, need, 2, logits + (size_t)s * h->n_classes * v0, buf, (hipStream_t)stream)) return rc;
    }
    return OAI_OK;
}

// What a tile must produce along one axis: its kept centre [ovl, tile-ovl) clipped to the part of the volume that
// Partition.assemble keeps (image_transforms.py:504 trims to the image, :509-513 zeroes a frame of `crop` voxels).
__host__ __device__ static void keep_interval(int t, int eff, int ovl, int size, int crop, int& lo, int& hi) {
    const int v0 = t * eff;                                   // volume coordinate of the kept centre's first voxel
    const int a = crop - v0 > 0 ? crop - v0 : 0;
    const int b = size - crop - v0 < eff ? size - crop - v0 : eff;
    lo = ovl + a;
    hi = ovl + b;                                             // hi <= lo: this tile contributes nothing
}

struct SegGeom {
    int eff[3], grid[3], ntiles;
};

static int seg_geometry(int D, int H, int W, const int tile[3], const int overlap[3], SegGeom& g) {
    const int size[3] = {D, H, W};
    for (int i = 0; i < 3; ++i) {
        OAI_CHECK_ARG(overlap[i] >= 0 && tile[i] - 2 * overlap[i] > 0, "overlap too large for the tile");
        g.eff[i] = tile[i] - 2 * overlap[i];
        g.grid[i] = (size[i] + g.eff[i] - 1) / g.eff[i];
    }
    g.ntiles = g.grid[0] * g.grid[1] * g.grid[2];
    return OAI_OK;
}

struct SegParams {          // everything tile_regions needs, by value (kernel argument)
    int size[3], tile[3], overlap[3], crop[3], eff[3], grid[3];
    int trimmed;
};

// need[layer] of tile t (z-major index), or all-empty boxes for a tile that contributes nothing
__host__ __device__ static void tile_regions(int t, const SegParams& p, Box need[18]) {
    const int idx[3] = {t / (p.grid[1] * p.grid[2]), (t / p.grid[2]) % p.grid[1], t % p.grid[2]};
    int lo[3], hi[3];
    bool dead = false;
    for (int i = 0; i < 3; ++i) {
        keep_interval(idx[i], p.eff[i], p.overlap[i], p.size[i], p.crop[i], lo[i], hi[i]);
        if (hi[i] <= lo[i]) dead = true;
        if (!p.trimmed) { lo[i] = p.overlap[i]; hi[i] = p.tile[i] - p.overlap[i]; }
    }
    plan_regions(p.tile, lo, hi, p.trimmed != 0, need);
    if (dead && p.trimmed)
        for (int k = 0; k < 18; ++k) for (int i = 0; i < 3; ++i) need[k].lo[i] = need[k].hi[i] = 0;
}

// device table [layer][n][6] of tiles [t0, t0+n): computed on the device (no host copy: graph-capturable);
// up-conv rows hold the INPUT box (the halved output box).  Behind the 18 layers: the three pieces of every own-cover layer's box (kTableRows)
__global__ void box_table_kernel(SegParams p, int t0, int n, int* __restrict__ table) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    Box need[18];
    tile_regions(t0 + t, p, need);
    for (int k = 0; k < 18; ++k) {
        int* row = table + ((size_t)k * n + t) * 6;
        const bool up = layer_kind(k) == 2;
        for (int i = 0; i < 3; ++i) {
            row[i] = up ? need[k].lo[i] / 2 : need[k].lo[i];
            row[3 + i] = up ? (need[k].hi[i] + 1) / 2 : need[k].hi[i];
        }
        const int slot = own_cover_slot(k);
        if (slot < 0) continue;
        Box piece[3];
        tile_cover(need[k], piece);
        for (int s = 0; s < 3; ++s) {
            int* prow = table + ((size_t)(18 + 3 * slot + s) * n + t) * 6;
            for (int i = 0; i < 3; ++i) { prow[i] = piece[s].lo[i]; prow[3 + i] = piece[s].hi[i]; }
        }
    }
}

static SegParams seg_params(int D, int H, int W, const int tile[3], const int overlap[3], const int* crop, const SegGeom& g, bool trimmed) {
    SegParams p;
    const int size[3] = {D, H, W};
    for (int i = 0; i < 3; ++i) {
        p.size[i] = size[i]; p.tile[i] = tile[i]; p.overlap[i] = overlap[i]; p.crop[i] = crop ? crop[i] : 0;
        p.eff[i] = g.eff[i]; p.grid[i] = g.grid[i];
    }
    p.trimmed = trimmed ? 1 : 0;
    return p;
}

// bytes of the two volume-wide tensors of the shared encoder pass, or 0 when its conditions do not hold for this geometry
static size_t shared_enc_bytes(const oai_unet* h, const int tile[3], const int overlap[3], const SegGeom& g, int P[3]) {
    if (!first_fusion_ok(h) || !h->opt_shared || h->L[EC1].cout % 16 != 0) return 0;
    const int blk[3] = {4, 8, 16};                                         // the main block shape must tile the padded volume and the tile exactly
    for (int i = 0; i < 3; ++i) {
        P[i] = g.eff[i] * g.grid[i] + 2 * overlap[i];
        // tile origins (multiples of eff) on block boundaries: a block of the pass lies inside or outside a tile, never across its start (scatter
        // copy-out), and pooling windows are aligned; overlap >= 4: dc2's skip read stays >= 2 voxels inside the tile
        if (tile[i] % blk[i] || P[i] % blk[i] || g.eff[i] % blk[i] || overlap[i] < 4 || tile[i] < 8) return 0;
    }
    const size_t pv = (size_t)P[0] * P[1] * P[2];
    if (pv * 128 >= (1ull << 32)) return 0;                                // 32-bit piece offsets inside the pass's own planes
    const size_t nch = (size_t)h->L[EC1].cout / 16;
    return (nch * (pv / 8) * 64 + 255) / 256 * 256;
}

size_t oai_segment_workspace_bytes(const oai_unet* h, int D, int H, int W, const int tile[3], const int overlap[3], int batch) {
    if (!h || !tile || !overlap || batch <= 0) return 0;
    SegGeom g;
    if (seg_geometry(D, H, W, tile, overlap, g)) return 0;
    int P[3];
    return workspace_bytes(h, tile[0], tile[1], tile[2], batch) + shared_enc_bytes(h, tile, overlap, g, P);
}

int oai_segment_tiles(oai_unet* h, const float* vol, int D, int H, int W, const int tile[3], const int overlap[3],
                      const int crop[3], int tile_begin, int tile_end, int out_mode, float* blocks, int batch,
                      void* ws, size_t ws_bytes, void* stream) {
    OAI_CHECK_ARG(h && vol && tile && overlap && blocks && ws, "oai_segment_tiles: null pointer");
    OAI_CHECK_ARG(D > 1 && H > 1 && W > 1, "oai_segment_tiles: volume axes must be > 1 (reflect padding)");
    OAI_CHECK_ARG(out_mode >= 0 && out_mode <= 2, "oai_segment_tiles: out_mode must be 0, 1 or 2");
    if (int rc = check_tile(tile[0], tile[1], tile[2])) return rc;
    SegGeom g;
    if (int rc = seg_geometry(D, H, W, tile, overlap, g)) return rc;
    OAI_CHECK_ARG(0 <= tile_begin && tile_begin <= tile_end && tile_end <= g.ntiles,
                  "oai_segment_tiles: tile range [%d,%d) outside [0,%d)", tile_begin, tile_end, g.ntiles);
    OAI_CHECK_ARG(batch > 0, "oai_segment_tiles: batch must be > 0");
    if (crop) for (int i = 0; i < 3; ++i) OAI_CHECK_ARG(crop[i] >= 0, "oai_segment_tiles: negative crop");
    float* buf[B_COUNT];
    int* table_dev;
    unsigned* lists[kOwnLayers];
    const size_t need_bytes = carve_workspace(h, tile[0], tile[1], tile[2], batch, ws, buf, table_dev, lists);
    if (need_bytes > ws_bytes)
        return set_error(OAI_ERR_WORKSPACE, "oai_segment_tiles: workspace %zu B < %zu B needed for batch %d", ws_bytes, need_bytes, batch);
    const size_t list_cap = block_list_capacity(tile[0], tile[1], tile[2], batch);
    const bool trimmed = diag_env("OAI_NO_TRIM", 0) == 0;
    hipStream_t st = (hipStream_t)stream;
    TileSource src{};
    src.vol = vol; src.tiles = nullptr; src.D = D; src.H = H; src.W = W;
    src.td = tile[0]; src.th = tile[1]; src.tw = tile[2];
    src.ez = g.eff[0]; src.ey = g.eff[1]; src.ex = g.eff[2];
    src.oz = overlap[0]; src.oy = overlap[1]; src.ox = overlap[2];
    src.gy = g.grid[1]; src.gx = g.grid[2];
    const size_t bvox = (size_t)g.eff[0] * g.eff[1] * g.eff[2];
    const SegParams sp = seg_params(D, H, W, tile, overlap, crop, g, trimmed);
    Box need[18];
    // ---- shared encoder pass (run_batch: once per batch over the z range its tiles cover), when the geometry and the workspace allow it
    SharedEnc se{};
    bool shared = false;
    if (trimmed && tile_end > tile_begin) {
        int P[3];
        const size_t sb = shared_enc_bytes(h, tile, overlap, g, P);
        if (sb && need_bytes + sb <= ws_bytes) {
            shared = true;
            se.SP0 = reinterpret_cast<float*>((char*)ws + need_bytes);     // after the carved tensors
            se.PD = P[0]; se.PH = P[1]; se.PW = P[2];
            se.vol = vol; se.D = D; se.H = H; se.W = W;
            for (int i = 0; i < 3; ++i) { se.grid[i] = g.grid[i]; se.eff[i] = g.eff[i]; se.overlap[i] = overlap[i]; }
        }
    }
    for (int c0 = tile_begin; c0 < tile_end; c0 += kMaxTilesPerTable) {
        const int nc = tile_end - c0 < kMaxTilesPerTable ? tile_end - c0 : kMaxTilesPerTable;
        box_table_kernel<<<cdiv(nc, 64), 64, 0, st>>>(sp, c0, nc, table_dev);
        OAI_CHECK_LAUNCH();
        for (int t = c0; t < c0 + nc; t += batch) {
            const int n = c0 + nc - t < batch ? c0 + nc - t : batch;
            // launch boxes of this batch = union over its tiles (host mirror of the same planning code)
            Box uni[18];
            for (int k = 0; k < 18; ++k) for (int i = 0; i < 3; ++i) { uni[k].lo[i] = 1 << 30; uni[k].hi[i] = 0; }
            OwnPlan own{};
            for (int j = 0; j < n; ++j) {
                tile_regions(t + j, sp, need);
                own_plan_add(own, need);
                for (int k = 0; k < 18; ++k) {
                    if (need[k].hi[0] <= need[k].lo[0]) continue;
                    for (int i = 0; i < 3; ++i) {
                        if (need[k].lo[i] < uni[k].lo[i]) uni[k].lo[i] = need[k].lo[i];
                        if (need[k].hi[i] > uni[k].hi[i]) uni[k].hi[i] = need[k].hi[i];
                    }
                }
            }
            if (uni[0].hi[0] == 0) continue;                 // every tile of the batch is dead
            // option "one_launch": the live-block lists of the own-cover layers that run as one launch for this batch, built on the device from the table
            if (h->opt_own_cover && h->sres && (h->opt_one_launch & 3)) {
                int mask = 0;
                for (int slot = 0; slot < kOwnLayers; ++slot) {
                    own.list[slot] = lists[slot];
                    own.list_len[slot] = one_launch_family(h, h->L[kOwnLayerOf[slot]]) ? one_launch_len(h, own.tile_nb.data(), n, slot, list_cap) : 0;
                    if (own.list_len[slot]) mask |= 1 << slot;
                }
                if (mask) {
                    block_list_kernel<<<kOwnLayers * kListParts, 256, 0, st>>>(table_dev, nc, t - c0, n, lists[0], (size_t)(lists[1] - lists[0]), (int)std::min<size_t>(list_cap, 1u << 30), mask);
                    OAI_CHECK_LAUNCH();
                }
            }
            src.tile_begin = t;
            if (int rc = run_batch(h, src, n, uni, out_mode, blocks + (size_t)(t - tile_begin) * h->n_classes * bvox,
                                   buf, st, table_dev, nc, t - c0, shared ? &se : nullptr, &own)) return rc;
        }
    }
    return OAI_OK;
}

double oai_unet_volume_flops(const oai_unet* h, int D, int H, int W, const int tile[3], const int overlap[3],
                             const int crop[3], int trimmed, int conv3_only) {
    if (!h || !tile || !overlap) return 0.0;
    SegGeom g;
    if (seg_geometry(D, H, W, tile, overlap, g)) return 0.0;
    double f = 0.0;
    Box need[18];
    const SegParams sp = seg_params(D, H, W, tile, overlap, crop, g, trimmed != 0);
    for (int t = 0; t < g.ntiles; ++t) {
        tile_regions(t, sp, need);
        for (int k = 0; k < 18; ++k) {
            if (conv3_only && !is_conv3_igemm(k)) continue;
            f += layer_flops(h, k, need[k]);
        }
    }
    return f;
}

int oai_unet_tile_costs(const oai_unet* h, int D, int H, int W, const int tile[3], const int overlap[3], const int crop[3],
                        double* costs_host, int n_tiles) {
    OAI_CHECK_ARG(h && tile && overlap && costs_host, "oai_unet_tile_costs: null pointer");
    SegGeom g;
    if (int rc = seg_geometry(D, H, W, tile, overlap, g)) return rc;
    OAI_CHECK_ARG(n_tiles == g.ntiles, "oai_unet_tile_costs: the volume has %d tiles, not %d", g.ntiles, n_tiles);
    Box need[18];
    const SegParams sp = seg_params(D, H, W, tile, overlap, crop, g, true);
    for (int t = 0; t < g.ntiles; ++t) {
        tile_regions(t, sp, need);
        double f = 0.0;
        for (int k = 0; k < 18; ++k) f += layer_flops(h, k, need[k]);
        costs_host[t] = f;
    }
    return OAI_OK;
}

// blocks of TZ x TY x TX on the grid of `launch` that the kernels start for a tile with box `tb` (their start test), each at its live z slices x TY x TX
static double started_block_voxels(const Box& launch, int TY, int TX, const Box& tb) {
    if (box_empty(launch)) return 0.0;
    Box b;
    for (int i = 0; i < 3; ++i) { b.lo[i] = std::max(launch.lo[i], tb.lo[i]); b.hi[i] = std::min(launch.hi[i], tb.hi[i]); }
    if (box_empty(b)) return 0.0;
    auto started = [&](int i, int T) { int c = 0; for (int o = launch.lo[i]; o < launch.hi[i]; o += T) c += !(o >= b.hi[i] || o + T <= b.lo[i]); return c; };
    const double yx = (double)started(1, TY) * started(2, TX) * TY * TX;
    double v = 0.0;
    for (int oz = launch.lo[0]; oz < launch.hi[0]; oz += 4) {
        if (oz >= b.hi[0] || oz + 4 <= b.lo[0]) continue;
        const int m_lo = std::max(0, b.lo[0] - oz), m_hi = std::min(4, b.hi[0] - oz);
        v += (m_lo == 0 ? m_hi : 4) * yx;
    }
    return v;
}

int oai_unet_cover_stats(int D, int H, int W, const int tile[3], const int overlap[3], const int crop[3], int batch, int layer,
                         double stats_host[3], int* pieces_host, int n_tiles) {
    OAI_CHECK_ARG(tile && overlap && stats_host, "oai_unet_cover_stats: null pointer");
    OAI_CHECK_ARG(batch > 0, "oai_unet_cover_stats: batch must be > 0");
    const bool up = layer >= 0 && layer < 18 && layer_kind(layer) == 2;
    OAI_CHECK_ARG(up || (layer >= 0 && layer < 18 && own_cover_slot(layer) >= 0), "oai_unet_cover_stats: layer %d is neither an own-cover conv layer nor an up-conv", layer);
    if (int rc = check_tile(tile[0], tile[1], tile[2])) return rc;
    SegGeom g;
    if (int rc = seg_geometry(D, H, W, tile, overlap, g)) return rc;
    OAI_CHECK_ARG(!pieces_host || n_tiles == g.ntiles, "oai_unet_cover_stats: the volume has %d tiles, not %d", g.ntiles, n_tiles);
    const SegParams sp = seg_params(D, H, W, tile, overlap, crop, g, true);
    auto in_box = [&](Box b) { if (up) for (int i = 0; i < 3; ++i) { b.lo[i] /= 2; b.hi[i] = (b.hi[i] + 1) / 2; } return b; };   // (up-convs: the input box, as the table rows)
    auto voxels = [](const Box& b) { return box_empty(b) ? 0.0 : (double)(b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]); };
    Box need[18];
    stats_host[0] = stats_host[1] = stats_host[2] = 0.0;
    for (int t0 = 0; t0 < g.ntiles; t0 += batch) {
        const int n = std::min(batch, g.ntiles - t0);
        Box uni;                                                             // the launch box of the batch, as oai_segment_tiles forms it
        for (int i = 0; i < 3; ++i) { uni.lo[i] = 1 << 30; uni.hi[i] = 0; }
        for (int j = 0; j < n; ++j) {
            tile_regions(t0 + j, sp, need);
            if (box_empty(need[layer])) continue;
            for (int i = 0; i < 3; ++i) { uni.lo[i] = std::min(uni.lo[i], need[layer].lo[i]); uni.hi[i] = std::max(uni.hi[i], need[layer].hi[i]); }
        }
        Box launch = in_box(uni);
        launch.lo[2] &= up ? ~0 : ~1;
        const Cover c = cover_box(launch, 8, 4, 4, false);                   // (launch_conv3_wino)
        for (int j = 0; j < n; ++j) {
            tile_regions(t0 + j, sp, need);
            const Box b = in_box(need[layer]);
            Box piece[3] = {b, {}, {}};
            stats_host[0] += voxels(b);
            if (up) {                                                        // rows of 128 per started workgroup (upconv2_igemm_sres)
                if (!box_empty(b) && !box_empty(launch)) {
                    const int ryx = (launch.hi[1] - launch.lo[1]) * (launch.hi[2] - launch.lo[2]), nvox = (launch.hi[0] - launch.lo[0]) * ryx;
                    for (int mb = 0; mb < cdiv(nvox, 128); ++mb) {
                        const int zf = launch.lo[0] + (mb * 128) / ryx, zl = launch.lo[0] + std::min(mb * 128 + 127, nvox - 1) / ryx;
                        if (!(zl < b.lo[0] || zf >= b.hi[0])) stats_host[1] += 128.0;
                    }
                    stats_host[2] += 128.0 * cdiv((int)voxels(b), 128);
                }
            } else {
                stats_host[1] += started_block_voxels(c.main, 8, 8, b);
                if (c.wr) stats_host[1] += started_block_voxels(c.xs, 16, 4, b);
                if (c.hr) stats_host[1] += started_block_voxels(c.ys, 4, 16, b);
                tile_cover(b, piece);
                for (int s = 0; s < 3; ++s) {
                    int nb[3];
                    piece_blocks(piece[s], s, nb);
                    if (nb[0]) stats_host[2] += (double)(piece[s].hi[0] - piece[s].lo[0]) * nb[1] * nb[2] * kWinoTY[s] * kWinoTX[s];   // (own origin: m_lo == 0, live slices add up to the extent)
                }
            }
            if (pieces_host) {
                int* row = pieces_host + (size_t)(t0 + j) * 24;
                for (int i = 0; i < 3; ++i) { row[i] = b.lo[i]; row[3 + i] = b.hi[i]; }
                for (int s = 0; s < 3; ++s) for (int i = 0; i < 3; ++i) { row[6 + 6 * s + i] = piece[s].lo[i]; row[9 + 6 * s + i] = piece[s].hi[i]; }
            }
        }
    }
    return OAI_OK;
}

int oai_unet_block_list(int D, int H, int W, const int tile[3], const int overlap[3], const int crop[3], int batch, int tile_begin, int n, int layer,
                        unsigned* entries_host, int capacity, int* n_entries, long long* workspace_offset) {
    OAI_CHECK_ARG(tile && overlap && n_entries, "oai_unet_block_list: null pointer");
    OAI_CHECK_ARG(layer >= 0 && layer < 18 && own_cover_slot(layer) >= 0, "oai_unet_block_list: layer %d is not an own-cover conv layer", layer);
    if (int rc = check_tile(tile[0], tile[1], tile[2])) return rc;
    SegGeom g;
    if (int rc = seg_geometry(D, H, W, tile, overlap, g)) return rc;
    OAI_CHECK_ARG(batch > 0 && n > 0 && n <= batch && tile_begin >= 0 && tile_begin + n <= g.ntiles,
                  "oai_unet_block_list: tiles [%d, %d + %d) are not a batch of at most %d of the volume's %d tiles", tile_begin, tile_begin, n, batch, g.ntiles);
    const SegParams sp = seg_params(D, H, W, tile, overlap, crop, g, true);
    const int slot = own_cover_slot(layer);
    OwnPlan own{};
    Box need[18];
    for (int j = 0; j < n; ++j) {                                            // (the walk of oai_segment_tiles over the batch)
        tile_regions(tile_begin + j, sp, need);
        own_plan_add(own, need);
    }
    const int len = block_list_len(own.tile_nb.data(), n, slot, block_list_capacity(tile[0], tile[1], tile[2], batch));
    *n_entries = len;
    if (workspace_offset) *workspace_offset = (long long)block_list_offset(tile[0], tile[1], tile[2], batch, slot);
    if (entries_host) {
        OAI_CHECK_ARG(capacity >= len, "oai_unet_block_list: %d entries do not fit the %d given", len, capacity);
        if (len > 0) block_list_host(own.tile_nb.data(), n, slot, entries_host);      // (0: the batch does not fit the entry format and keeps its three launches)
    }
    return OAI_OK;
}

int oai_stitch_blocks(const float* blocks, int ncls, int D, int H, int W, const int tile[3], const int overlap[3],
                      const int crop[3], float* maps, void* stream) {
    StitchRanges rg{};
    return stitch_impl(blocks, ncls, D, H, W, tile, overlap, crop, maps, stream, rg);
}

int oai_stitch_blocks_ranged(const float* blocks, int ncls, int D, int H, int W, const int tile[3], const int overlap[3],
                             const int crop[3], const int* bounds_host, int n_ranges, int slot_stride, float* maps, void* stream) {
    OAI_CHECK_ARG(bounds_host, "oai_stitch_blocks_ranged: null pointer");
    OAI_CHECK_ARG(n_ranges >= 1 && n_ranges <= 64, "oai_stitch_blocks_ranged: 1..64 ranges, got %d", n_ranges);
    StitchRanges rg{};
    rg.n = n_ranges; rg.stride = slot_stride;
    OAI_CHECK_ARG(bounds_host[0] == 0, "oai_stitch_blocks_ranged: the ranges must start at tile 0");
    for (int r = 0; r <= n_ranges; ++r) {
        rg.bound[r] = bounds_host[r];
        if (r) OAI_CHECK_ARG(bounds_host[r] >= bounds_host[r - 1] && bounds_host[r] - bounds_host[r - 1] <= slot_stride,
                             "oai_stitch_blocks_ranged: range %d is not ascending or longer than the slot stride %d", r - 1, slot_stride);
    }
    if (tile && overlap) {
        long long nt = 1;
        const int size[3] = {D, H, W};
        for (int i = 0; i < 3; ++i) { const int e = tile[i] - 2 * overlap[i]; if (e > 0) nt *= (size[i] + e - 1) / e; }
        OAI_CHECK_ARG(bounds_host[n_ranges] == nt, "oai_stitch_blocks_ranged: the ranges cover %d tiles, the volume has %lld", bounds_host[n_ranges], nt);
    }
    return stitch_impl(blocks, ncls, D, H, W, tile, overlap, crop, maps, stream, rg);
}

}  // extern "C"
