// The direct (implicit-GEMM) k3 conv kernels and their launchers: conv3_igemm_f32, conv3_igemm_bf16s, conv3_igemm_sres2, and conv3_igemm_sres on its
// 32x32x16 taps.  No other file names these kernels: their instantiations are emitted here.  The M16 half of conv3_igemm_sres (16x16x32 tap pairs, as many
// instantiations again) is emitted by unet_direct_m16.hip and reached through launch_sres_m16, so that the two halves compile side by side.
#include "unet_host.h"
#include "unet_sres2.h"

namespace oai {

// conv3_igemm_sres2 in its variant `var`: 0 in the production library; -DOAI_DIAG builds also have the diagnostic variants 1..10 (OAI_WIDE_VAR)
template <int RX, int RY, int WY, int WX, int V = 0>
static void launch_sres2(int var, unsigned grid, hipStream_t st, const ConvArgs& a, const unsigned char* zero_rec) {
#ifdef OAI_DIAG
    if constexpr (V < 10)
        if (var != V) return launch_sres2<RX, RY, WY, WX, V + 1>(var, grid, st, a, zero_rec);
#endif
    conv3_igemm_sres2<RX, RY, WY, WX, V><<<grid, 512, 0, st>>>(a, zero_rec);
}

template <int MREP, int KC, int RX, int RY, int WY, int WX>
static int launch_conv3_shape(const oai_unet* h, ConvArgs a, const Box& box, int ntiles, hipStream_t st, int mrep_override = 0) {   // a.boxes set by the caller
    for (int i = 0; i < 3; ++i) { a.lo[i] = box.lo[i]; a.hi[i] = box.hi[i]; }
    if (box.hi[0] <= box.lo[0] || box.hi[1] <= box.lo[1] || box.hi[2] <= box.lo[2]) return OAI_OK;
    // conv3_igemm_sres2 (unet_sres2.h): main shape of the default split-resident configuration, 128 couts per workgroup
    // ... when the launch is at least four rounds of its one-workgroup-per-CU blocks (ec6 of the reference network: 2.5 rounds, 13 % slower
    // than as twice as many 4-wave workgroups)
    const int sres_mrep = mrep_override ? mrep_override : h->sres_mrep;       // z slices per block of the split-resident kernel for THIS launch
    constexpr bool kMainShape = RX == 16 && RY == 2 && WY == 4 && WX == 1;
    // + the 4-row y strip (dc5: 2.27 -> 1.89 ms); the 4-column x strip <4,8,4,1> measured slower there (2.05 -> 2.30 ms) and stays on the 4-wave kernel
    constexpr bool kWideShape = kMainShape || (RX == 16 && RY == 2 && WY == 2 && WX == 2);
    bool wide = KC == 8 && kWideShape && h->sres && h->opt_wide && sres_mrep == 4 && !a.first_w && !a.head_w && a.Cout % 128 == 0;
    if (wide && h->opt_wide == 1) {
        const size_t nwg = (size_t)ntiles * cdiv(box.hi[0] - box.lo[0], 4) * cdiv(box.hi[1] - box.lo[1], WY * RY) * cdiv(box.hi[2] - box.lo[2], WX * RX) * (a.Cout / 128);
        wide = nwg >= (kMainShape ? 1024 : 512);
    }
    if (wide) a.ncb = a.Cout / 128;
    const bool bf = KC == 8 && h->precision != OAI_PREC_F32;       // the split kernels use 2 z slices per block (4: split-resident)
    // exact fp32: two z slices per block -- the registers of the other two hold the per-chunk partial sums of its two-level accumulation (conv3_igemm_f32)
    constexpr int kF32Mrep = MREP > 2 ? 2 : MREP;
    a.nbz = cdiv(box.hi[0] - box.lo[0], bf ? (h->sres ? sres_mrep : 2) : kF32Mrep);
    a.nby = cdiv(box.hi[1] - box.lo[1], WY * RY);
    a.nbx = cdiv(box.hi[2] - box.lo[2], WX * RX);
    unsigned grid = (unsigned)((size_t)ntiles * a.nbz * a.nby * a.nbx * a.ncb);
    if (KC == 8 && h->sres) grid = xcd_deal(h, grid, a.nblocks, a.xcd_group);
    if (int rc = launch_begin(h, st)) return rc;
    if (KC == 8 && h->sres) {
        // (diagnostic builds: OAI_ONE_WG=1 asks for 24 KB of unused dynamic LDS, which leaves room for ONE workgroup per CU -- the tap
        // stream of a wave that has the SIMD to itself, scripts/stamp_phases.py)
        static const int one_wg = diag_env("OAI_ONE_WG", 0);
        bool done = false;
        // the 16x16x32 tap pairs (option "m16"): a per-LAYER decision -- never for a layer that the bit-identical 128-cout form conv3_igemm_sres2 may
        // take for some of its launches (that choice depends on the launch size) -- and every shape of the kernel has the variant
        const bool m16 = h->opt_m16 && a.wpanel16 && a.Cout % 128 != 0 && !one_wg;
        if (m16) a.wpanel = a.wpanel16;
        if constexpr (RX == 16 && RY == 2 && WY == 4 && WX == 1) {
            if (a.first_w) {                                         // ec0 fused into ec1's halo staging (first_fusable guarantees mrep 4, no strips)
                if (m16) launch_sres_m16<RX, RY, WY, WX>(4, true, grid, st, a, h->zero_rec);
                else conv3_igemm_sres<4, RX, RY, WY, WX, true><<<grid, 256, 0, st>>>(a, h->zero_rec);
                done = true;
            }
        }
        if constexpr (kWideShape) {
            if (wide) {
                static const int var = diag_env("OAI_WIDE_VAR", 0);         // -DOAI_DIAG builds only; constant 0 otherwise
                launch_sres2<RX, RY, WY, WX>(var >= 1 && var <= 10 ? var : 0, grid, st, a, h->zero_rec);
                done = true;
            }
        }
        if (done) { }
        else if (a.first_w) return set_error(OAI_ERR_ARG, "fused ec0 asked of a tile shape that has no such kernel");
        else if (m16) launch_sres_m16<RX, RY, WY, WX>(sres_mrep, false, grid, st, a, h->zero_rec);
        else if (sres_mrep == 4) conv3_igemm_sres<4, RX, RY, WY, WX><<<grid, 256, one_wg ? 24 * 1024 : 0, st>>>(a, h->zero_rec);
        else conv3_igemm_sres<2, RX, RY, WY, WX><<<grid, 256, 0, st>>>(a, h->zero_rec);
    }
    else if (KC == 8 && h->precision == OAI_PREC_BF16X3) conv3_igemm_bf16s<2, false, 2, RX, RY, WY, WX><<<grid, 256, 0, st>>>(a);
    else if (KC == 8 && h->precision == OAI_PREC_BF16X6) conv3_igemm_bf16s<3, false, 2, RX, RY, WY, WX><<<grid, 256, 0, st>>>(a);
    else if (KC == 8 && h->precision == OAI_PREC_FP16X3) conv3_igemm_bf16s<2, true, 2, RX, RY, WY, WX><<<grid, 256, 0, st>>>(a);
    else conv3_igemm_f32<kF32Mrep, KC, RX, RY, WY, WX><<<grid, 256, 0, st>>>(a);
    return launch_end(h, st);
}

// the cover of the direct kernels: main tiles of 8 x 16
static Cover direct_cover(const oai_unet* h, const Box& box) { return cover_box(box, 16, 4, 8, h->variant == 2); }

// what fusing ec0 into ec1 asks of the configuration: the default split-resident kernel and the reference's channel counts (1 -> 32 -> ...)
bool first_fusion_ok(const oai_unet* h) {
    return h->sres && h->fuse_first && h->variant == 0 && h->sres_mrep == 4 && h->L[EC0].cout == 32 && h->L[EC1].c0 == 32;
}
// ec0 can be computed inside ec1's halo staging (conv3_igemm_sres<..., FIRST>) when ec1 runs as ONE launch of the main shape
bool first_fusable(const oai_unet* h, const Box& ec1_box) {
    if (!first_fusion_ok(h)) return false;
    const Cover c = direct_cover(h, ec1_box);
    return c.hr == 0 && c.wr == 0;
}

// one launch of ONE given tile shape over `box` (the faces of the per-tile shell pass, where launch_conv3_direct's main + strips cover does not fit)
// `pool_only` (main shape): the max-pooled tensor is all this launch leaves behind -- fused pool into pool_only, 2 z slices per block (both
// slices of a block are then inside the 2-voxel face), the copy-out of the layer's own output suppressed through an empty store box
template <int RX, int RY, int WY, int WX>
int launch_conv3_one(const oai_unet* h, const Layer& L, const float* s0, float* out, const int dims[3], const Box& box, int ntiles,
                     hipStream_t st, const int* boxes, float* pool_only) {
    ConvArgs a;
    if (int rc = fill_conv_args(h, L, s0, nullptr, out, dims, {.boxes = boxes, .pool_out = pool_only}, a)) return rc;
    if (pool_only) { a.store_boxes = boxes; a.store_grow = -(1 << 20); }          // consumer box "grown" by -2^20: nothing of the output tensor is written
    return launch_conv3_shape<4, 8, RX, RY, WY, WX>(h, a, box, ntiles, st, pool_only ? 2 : 0);
}
template int launch_conv3_one<16, 2, 4, 1>(const oai_unet*, const Layer&, const float*, float*, const int[3], const Box&, int, hipStream_t, const int*, float*);
template int launch_conv3_one<16, 2, 1, 4>(const oai_unet*, const Layer&, const float*, float*, const int[3], const Box&, int, hipStream_t, const int*, float*);
template int launch_conv3_one<2, 16, 4, 1>(const oai_unet*, const Layer&, const float*, float*, const int[3], const Box&, int, hipStream_t, const int*, float*);

// A conv layer through the direct kernels: the main launch of 4 x 8 x 16 blocks and the strips of direct_cover, each with the shape that fits it
int launch_conv3_direct(const oai_unet* h, const ConvArgs& a, const Box& box, int ntiles, hipStream_t st) {
#ifdef OAI_DIAG
    // OAI_CONV_VARIANT 1: the KC = 16 kernel, in diagnostic builds only.  launch_conv3 tests the Winograd arms first; a handle with variant != 0 never takes
    // them because oai_unet_set_precision keeps it in exact fp32 (no h->sres) and the fp32 Winograd gate asks for variant == 0: keep both when editing the gates.
    if (h->variant == 1) return launch_conv3_shape<2, 16, 16, 2, 4, 1>(h, a, box, ntiles, st);
#endif
    const Cover c = direct_cover(h, box);
    if (int rc = launch_conv3_shape<4, 8, 16, 2, 4, 1>(h, a, c.main, ntiles, st)) return rc;
    if (c.wr) {
        const int rc = c.wr <= 2 ? launch_conv3_shape<4, 8, 2, 16, 4, 1>(h, a, c.xs, ntiles, st)
                     : c.wr <= 4 ? launch_conv3_shape<4, 8, 4, 8, 4, 1>(h, a, c.xs, ntiles, st)
                                 : launch_conv3_shape<4, 8, 8, 4, 4, 1>(h, a, c.xs, ntiles, st);
        if (rc) return rc;
    }
    if (!c.hr) return OAI_OK;
    return c.hr <= 2 ? launch_conv3_shape<4, 8, 16, 2, 1, 4>(h, a, c.ys, ntiles, st) : launch_conv3_shape<4, 8, 16, 2, 2, 2>(h, a, c.ys, ntiles, st);
}

}  // namespace oai
