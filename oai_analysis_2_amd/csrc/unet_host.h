// What the translation units of the segmentation path's host side share: the network handle, the boxes and covers of the tile
// geometry, and the functions that cross files.  Each kernel family is emitted by the file that holds its launchers:
//   unet.hip         geometry (regions, covers, block lists, box table), the schedule (run_batch), options, the C ABI
//   unet_pack.hip    weight ingest: panels, number formats, uploads; no kernel
//   unet_direct.hip  conv3_igemm_f32 / _bf16s / _sres2 and conv3_igemm_sres on 32x32x16 taps
//   unet_direct_m16.hip  conv3_igemm_sres<..., M16> (16x16x32 tap pairs)
//   unet_wino.hip    conv3_wino_sres, conv3_wino_list1 / 2, conv3_wino_f32
//   unet_small.hip   up-conv, pool, ec0, head, pooled gather, stitch, range flag -- and every kernel of the headers that is no template
// Nothing with state lives here: a function-local cache or a global has its one definition in one of the files.
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"
#include "unet_kernels.h"

namespace oai {

enum LayerId { EC0, EC1, EC2, EC3, EC4, EC5, EC6, EC7, DC9, DC8, DC7, DC6, DC5, DC4, DC3, DC2, DC1, DC0 };
__host__ __device__ static inline int layer_level(int k) { const int v[18] = {0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0}; return v[k]; }   // OUTPUT level
__host__ __device__ static inline int layer_kind(int k) { const int v[18] = {0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 1, 2, 1, 1, 2, 1, 1, 3}; return v[k]; }

struct Layer {
    int kind = 0, cin = 0, cout = 0;
    int c0 = 0, c1 = 0;                 // concat split of cin (c1 = skip channels)
    float4* panel = nullptr;            // MFMA weight panel (kinds 0,1,2 except ec0)
    float4* panel_bf[3] = {nullptr, nullptr, nullptr};   // split panels of the k3 layers: bf16 x2 terms, bf16 x3 terms, fp16 x2 terms
    // fp16x3 epilogue affine (refresh_fp16_affine): scale / ws * 2^(e_out - e_in0), shift * 2^e_out with ws = the fp16 panel's per-cout
    // power-of-two weight scale and e = the activation exponents of the layer's output / first input tensor (oai_unet::act_exp)
    float* scale_f16 = nullptr;
    float* shift_f16 = nullptr;
    float* plain_f16 = nullptr;         // dc0 in fp16x3: head weights * 2^-e(dc1)
    std::vector<float> ws;              // per-cout weight scale of the fp16 panel (exact powers of two)
    int rel1 = 0;                       // exponent folded into the source-1 (skip) weights of the current fp16 panel: e(src0) - e(src1)
    size_t panel_f16_floats = 0;
    float4* panel_wino_f32 = nullptr;   // fp32 panel of conv3_wino_f32 (pack_wino_f32_panel): the x axis in Winograd F(2,3) form, exact-fp32 path
    float4* panel_wino = nullptr;       // fp16 panel of conv3_wino_sres (pack_wino_panel): the x axis in Winograd F(2,3) form; packed with the same ws / rel1
    size_t panel_wino_floats = 0;
    float4* panel_wino16 = nullptr;     // the same weights laid out for the 16x16x32 taps of conv3_wino_sres<..., M16> (pack_wino16_panel; Cout % 128 == 0 only)
    size_t panel_wino16_floats = 0;
    float4* panel_m16 = nullptr;        // the fp16 panel laid out for the 16x16x32 tap pairs of conv3_igemm_sres<..., M16> (pack_conv3_m16_panel): same values as panel_bf[2]
    size_t panel_m16_floats = 0;
    std::vector<float> wk_host;         // canonical [27][cin][cout] weights of the k3 layers (for re-packing)
    std::vector<float> scale_host, shift_host, plain_host;
    float* plain = nullptr;             // ec0: [27][cout]; dc0: [ncls][cin]
    float* scale = nullptr;
    float* shift = nullptr;
};

}  // namespace oai

struct oai_unet {
    oai::Layer L[18];
    int variant = 0;                    // 0: MREP4/KC8, 1: MREP2/KC16
    int precision = OAI_PREC_F32;
    int* range_flag = nullptr;          // device word set by the split-fp16 kernels when an activation exceeds fp16's range
    unsigned* census = nullptr;         // [18][16] float bits: max |stored activation| per layer since the last reset (census_note)
    int* eval_out = nullptr;            // device scratch of oai_unet_range_flag
    // Per-tensor activation exponents of the fp16x3 path: layer k stores x * 2^act_exp[k].  fp16's low split term needs |x| >= 2^-3 to be
    // normal; below that the pair (h0, h1) has an ABSOLUTE error floor of 2^-25, so a tensor whose values sit near 2^-10 would carry
    // 1e-5 relative error.  Calibration (oai_unet_calibrate_step) puts every layer's maximum in [2^10, 2^11): 5 bits of
    // headroom below 65504 and a floor of 2^-35 of the maximum.  Exact: powers of two fold into the epilogue affine and the panels.
    int act_exp[18] = {0};
    bool calibrated = false;
    // The tuning options and their defaults.  What each one does is written once, where it is set: kIntOptions / oai_unet_set_option.
    int opt_wino_f32 = 1;               // option "winograd_f32"
    int opt_first_blocks = 24;          // option "first_blocks"
    int opt_up_nbw = 0;                 // option "up_nbw"
    int opt_own_cover = 1;              // option "own_cover"
    int opt_one_launch = 1;             // option "one_launch"
    int opt_shared = 1;                // option "shared_enc"
    int opt_wide = 1;                   // option "wide"
    int opt_wino = 19;                  // option "winograd"
    int opt_wino_layers = 0x3FFFF;      // option "winograd_layers"
    int opt_m16 = 1;                    // option "m16"
    int opt_m16_layers = 0x3FFFF;       // option "m16_layers"
    int opt_dead_stores = 1;            // option "dead_stores"
    int opt_census = 1;                 // option "census"
    int xcd_group = 32;                 // option "xcd_group"
    int fuse_first = 1;                 // option "fuse_first"
    int sres_mrep = 4;                  // option "sres_mrep"
    bool opt_sres = true;               // option "sres": fp16x3 uses the split-resident kernels
    bool sres = false;                  // fp16x3 runs split-resident (activations stored as fp16 term pairs, unet_sres.h)
    unsigned char* zero_rec = nullptr;  // 64 zero bytes: source of halo voxels outside the tile for the LDS-DMA staging
    int n_classes = 0;
    std::vector<void*> allocs;
    bool profile = false;
    std::vector<hipEvent_t> ev_pool;      // reused start/stop pairs
    size_t ev_used = 0;
};

namespace oai {

struct Box { int lo[3], hi[3]; };

__host__ __device__ static void full_box(Box& b, const int dims[3]) { for (int i = 0; i < 3; ++i) { b.lo[i] = 0; b.hi[i] = dims[i]; } }
__host__ __device__ static inline bool box_empty(const Box& b) { return b.hi[0] <= b.lo[0] || b.hi[1] <= b.lo[1] || b.hi[2] <= b.lo[2]; }

// One conv layer = the main launch over the part of the output box that 8 x `xunit` (y, x) tiles cover exactly, plus up to two thin remainder
// strips computed with tile shapes that fit them (trimmed boxes are e.g. 18 x 98 x 98): the x strip = all y rows, the last wr columns; the y strip =
// the last hr rows, main columns only.  A remainder of more than tall_y rows / tall_x columns is cheaper as one more row / column of main tiles.
// hr == wr == 0: the main launch covers the whole box (also when the box is smaller than one main tile in y or x, or `no_strips`).
struct Cover { Box main, xs, ys; int hr, wr; };
__host__ __device__ static Cover cover_box(const Box& box, int xunit, int tall_y, int tall_x, bool no_strips) {
    const int ry = box.hi[1] - box.lo[1], rx = box.hi[2] - box.lo[2], ny = ry / 8, nx = rx / xunit;
    Cover c{box, box, box, ry - 8 * ny, rx - xunit * nx};
    if (no_strips || ny == 0 || nx == 0) c.hr = c.wr = 0;
    if (c.hr > tall_y) c.hr = 0;
    if (c.wr > tall_x) c.wr = 0;
    if (c.hr) c.main.hi[1] = box.lo[1] + 8 * ny;
    if (c.wr) c.main.hi[2] = box.lo[2] + xunit * nx;
    c.xs.lo[2] = c.main.hi[2];
    c.ys.lo[1] = c.main.hi[1]; c.ys.hi[2] = c.main.hi[2];
    return c;
}

// The layers whose blocks sit on every tile's OWN cover (option "own_cover"): the trimmed decoder convs dc8, dc7, dc5, dc4, dc2 (own_cover_slot)
constexpr int kOwnLayers = 5;
enum Buf { B_E0, B_SYN0, B_P0, B_E2, B_SYN1, B_P1, B_E4, B_SYN2, B_P2, B_E6, B_E7, B_U9, B_D8, B_D7, B_U6, B_D5, B_D4, B_U3, B_D2, B_D1, B_COUNT };

// what run_batch needs of the host's walk over a batch's tiles for option "own_cover": the grid of every shape of every own-cover layer (the largest
// block counts of any tile, per axis), the largest input box of every up-conv in voxels, and every tile's own block counts [tile][slot][shape][3]
// (all 0 for a dead tile), from which balanced_xcd_group deals a launch
// list / list_len (option "one_launch"): the device lists of the layers that run as one launch for this batch, 0 entries = three launches (one_launch_len)
struct OwnPlan { int nb[kOwnLayers][3][3]; int up_nvox[18]; std::vector<int> tile_nb; const unsigned* list[kOwnLayers]; int list_len[kOwnLayers]; };
// one own-cover layer of one batch, as launch_conv3_wino takes it: the device rows of the three pieces, their grids and XCD dealing granularities (0: the option's)
// `list` (option "one_launch"): the layer's live-block list on the device and its length, or null / 0 = one launch per shape
struct OwnCover { const int* rows[3]; int nb[3][3]; int xcd_group[3]; const unsigned* list; int list_len; };

// shared encoder pass: where the copy-out of the volume-wide ec1 scatters its voxels (ConvArgs::sc_*)
struct Scatter { const int* boxes; int ntiles, tile0; int g[3], e[3], t[3]; };

// the tensors and the geometry of the shared encoder pass (run_batch says what the pass does)
struct SharedEnc {
    float* SP0;                         // [cout / 16 chunks][PD / 2][PH / 2][PW / 2]: the max-pooled ec1 of the padded volume
    int PD, PH, PW;                     // reflect-padded volume = eff * grid + 2 * overlap
    const float* vol; int D, H, W;      // the volume itself (the pass gathers it with Partition's reflect padding)
    int grid[3], eff[3], overlap[3];
};

// What a conv layer's launch may take beyond its tensors; a call names what it sets.  boxes: the per-tile box rows of the layer; pool_out: the fused
// MaxPool3d(2); head: the fused dc0 fields (see ConvArgs); first: ec0 fused into the layer's staging (first_fusable); store_boxes: the consumer's rows
// (option "dead_stores"); sc: the scatter of the shared encoder pass; oc: the layer's own cover (option "own_cover").
struct ConvOpt {
    const int* boxes = nullptr;
    float* pool_out = nullptr;
    const ConvArgs* head = nullptr;
    const TileSource* first = nullptr;
    const int* store_boxes = nullptr;
    const Scatter* sc = nullptr;
    const OwnCover* oc = nullptr;
};

// tensors a layer reads: its first source is the previous layer of the schedule (a pooled tensor keeps its producer's exponent);
// dc8 / dc5 / dc2 also read the skips ec5 / ec3 / ec1
static inline int layer_src0(int k) { return k - 1; }
static inline int layer_src1(int k) { return k == DC8 ? EC5 : k == DC5 ? EC3 : k == DC2 ? EC1 : -1; }

// per-layer accessors: a layer's index in the schedule, its bit of a layer mask (options "winograd_layers", "m16_layers"), its 16 census words (null: option
// "census" 0 -- callers add their own h->sres condition)
static inline int layer_id(const oai_unet* h, const Layer& L) { return (int)(&L - h->L); }
static inline bool layer_bit(const oai_unet* h, int mask, const Layer& L) { return (mask >> layer_id(h, L)) & 1; }
static inline unsigned* census_of(const oai_unet* h, int k) { return h->opt_census ? h->census + 16 * k : nullptr; }

// the grid of an elementwise kernel: one thread per element in blocks of 256, at most `cap` blocks (the kernels walk the rest with a grid stride)
static inline unsigned capped_blocks(size_t total, size_t cap) { return (unsigned)std::min<size_t>((total + 255) / 256, cap); }

// ---- unet.hip
int launch_begin(const oai_unet* h, hipStream_t st);
int launch_end(const oai_unet* h, hipStream_t st);
unsigned xcd_deal(const oai_unet* h, unsigned grid, int& nblocks, int& xcd_group, int group = 0);
int fill_conv_args(const oai_unet* h, const Layer& L, const float* s0, const float* s1, float* out, const int dims[3], const ConvOpt& o, ConvArgs& a);
int block_list_len(const int* tile_nb, int ntiles, int slot, size_t capacity);
#ifdef OAI_DIAG
unsigned long long* layer_stamps(const oai_unet* h, const Layer& L);
#endif

// ---- unet_pack.hip
int conv_kc(int variant);
std::vector<float> canonical_k3(const oai_layer_params& p);
std::vector<float> pack_conv3_panel(const std::vector<float>& wk, int C0, int C1, int Cout, int KC);
std::vector<float> pack_wino_f32_panel(const std::vector<float>& wk, int C0, int C1, int Cout);
std::vector<float> pack_conv3_panel_bf(const std::vector<float>& wk, int C0, int C1, int Cout, int NS,
                                       bool fp16 = false, const std::vector<float>* wscale = nullptr, float src1_factor = 1.0f);
std::vector<float> pack_up_panel(const oai_layer_params& p);
template <typename T>
int upload(oai_unet* h, const std::vector<float>& v, T** dst);      // (instantiated for float and float4)
int pack_wino_layer(oai_unet* h, int k);
int pack_fp16_layer(oai_unet* h, int k);
int refresh_fp16_affine(oai_unet* h);

// ---- unet_direct.hip, unet_direct_m16.hip
// conv3_igemm_sres<mrep, RX, RY, WY, WX, first, M16 = true>: the direct split-resident kernel on the 16x16x32 tap pairs, emitted by unet_direct_m16.hip for the
// six block shapes of launch_conv3_direct / launch_conv3_one (`first`: the main shape only)
template <int RX, int RY, int WY, int WX>
void launch_sres_m16(int mrep, bool first, unsigned grid, hipStream_t st, const ConvArgs& a, const unsigned char* zero_rec);
bool first_fusion_ok(const oai_unet* h);
bool first_fusable(const oai_unet* h, const Box& ec1_box);
int launch_conv3_direct(const oai_unet* h, const ConvArgs& a, const Box& box, int ntiles, hipStream_t st);
// (instantiated for the three face shapes of the per-tile shell pass: <16, 2, 4, 1>, <16, 2, 1, 4>, <2, 16, 4, 1>)
template <int RX, int RY, int WY, int WX>
int launch_conv3_one(const oai_unet* h, const Layer& L, const float* s0, float* out, const int dims[3], const Box& box, int ntiles,
                     hipStream_t st, const int* boxes, float* pool_only = nullptr);

// ---- unet_wino.hip
int wino_groups(const oai_unet* h, int cout, int TY);
int one_launch_family(const oai_unet* h, const Layer& L);
int one_launch_len(const oai_unet* h, const int* tile_nb, int ntiles, int slot, size_t capacity);
bool wino_pool_box(const Box& box, const int dims[3]);
int launch_conv3_wino(const oai_unet* h, const Layer& L, const ConvArgs& a, Box box, int ntiles, hipStream_t st, const OwnCover* oc = nullptr);
int launch_conv3_wino_f32(const oai_unet* h, const Layer& L, const ConvArgs& a, Box box, int ntiles, hipStream_t st);

// ---- unet_small.hip
int launch_up(const oai_unet* h, const Layer& L, const float* src, float* out, const int in_dims[3], const Box& out_need,
              int ntiles, hipStream_t st, const int* in_boxes = nullptr, int own_nvox = 0);
int launch_pool(const oai_unet* h, const float* in, float* out, const int dims[3], int C, int ntiles, hipStream_t st, int shell_only = 0);
int launch_first(const oai_unet* h, const TileSource& src, float* e0, int ntiles, hipStream_t st);
int launch_first_shell(const oai_unet* h, const TileSource& src, float* e0, const int dims[3], int ntiles, hipStream_t st);
int launch_pooled_gather(const oai_unet* h, const SharedEnc& se, const TileSource& src, float* p0, const int dims[3], int ntiles, hipStream_t st);
int launch_head(const oai_unet* h, const float* in, const int dims[3], const Box& keep, const int origin[3], const int eff[3], int out_mode,
                float* blocks_out, const int* boxes, int ntiles, hipStream_t st);
int launch_range_eval(const oai_unet* h, int* dst, int reset, hipStream_t st);
int launch_range_state(const oai_unet* h, int* dst, hipStream_t st);
int launch_range_flag_from_state(const int* state, int* dst, hipStream_t st);
int stitch_impl(const float* blocks, int ncls, int D, int H, int W, const int tile[3], const int overlap[3],
                const int crop[3], float* maps, void* stream, const StitchRanges& rg);

}  // namespace oai
