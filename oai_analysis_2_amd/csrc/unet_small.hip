// The small kernels of the segmentation path and their launches: k2s2 up-conv, max-pool, ec0, head, the pooled gather of the shared encoder
// pass, stitch, and the range flag.  This is the one file that emits the kernels of unet_kernels.h / unet_sres.h that are no templates.
#define OAI_UNET_PLAIN_KERNELS 1
#include "unet_host.h"
#include "unet_sres.h"

namespace oai {

int launch_up(const oai_unet* h, const Layer& L, const float* src, float* out, const int in_dims[3], const Box& out_need,
              int ntiles, hipStream_t st, const int* in_boxes, int own_nvox) {
    UpArgs a;
    a.boxes = in_boxes;
    a.range_flag = h->range_flag;
    a.zero = h->zero_rec;
#ifdef OAI_DIAG
    a.stamps = layer_stamps(h, L);
#endif
    const bool split = h->precision == OAI_PREC_FP16X3 && L.panel_bf[2];
    a.src = src; a.Cin = L.cin; a.out = out; a.Cout = L.cout;
    a.wpanel = split ? L.panel_bf[2] : L.panel;
    a.scale = split ? L.scale_f16 : L.scale;
    a.shift = split ? L.shift_f16 : L.shift;
    a.census = h->sres ? census_of(h, layer_id(h, L)) : nullptr;
    a.D = in_dims[0]; a.H = in_dims[1]; a.W = in_dims[2];
    for (int i = 0; i < 3; ++i) { a.lo[i] = out_need.lo[i] / 2; a.hi[i] = (out_need.hi[i] + 1) / 2; }
    const int nvox = (a.hi[0] - a.lo[0]) * (a.hi[1] - a.lo[1]) * (a.hi[2] - a.lo[2]);
    a.nmb = cdiv(nvox, split && h->sres ? 128 : 64);       // voxels per workgroup: 128 in the split-resident kernel
    a.nnb = cdiv(8 * L.cout, 256);
    a.relu = 1;
    if (split && h->sres) {
        // option "own_cover": a tile's workgroups list the voxels of its own input box -- as many row blocks as the batch's largest tile box has
        if (own_nvox > 0 && in_boxes) { a.own_box = 1; a.nmb = cdiv(own_nvox, 128); }
        // column blocks per workgroup (round 6): as many as leave >= 16 workgroups per workgroup slot of the chip (256 CUs x 2); narrow test networks
        // (the dword-store path of the kernel) keep one; option "up_nbw": 0 = this rule, n = at most n
        a.nbw = 1;
        if (L.cout % 16 == 0 && h->opt_up_nbw > 1) a.nbw = std::min(h->opt_up_nbw, a.nnb);
        else if (L.cout % 16 == 0 && h->opt_up_nbw == 0) {
            a.nbw = a.nnb;
            while (a.nbw > 1 && (size_t)ntiles * a.nmb * cdiv(a.nnb, a.nbw) < 8192) a.nbw = (a.nbw + 1) / 2;
        }
        const unsigned grid = xcd_deal(h, (unsigned)((size_t)ntiles * a.nmb * cdiv(a.nnb, a.nbw)), a.nblocks, a.xcd_group);   // same dealing as the conv kernels'
        upconv2_igemm_sres<<<grid, 256, 0, st>>>(a);
    }
    else if (split) upconv2_igemm<true><<<(unsigned)((size_t)ntiles * a.nmb * a.nnb), 256, 0, st>>>(a);
    else upconv2_igemm<false><<<(unsigned)((size_t)ntiles * a.nmb * a.nnb), 256, 0, st>>>(a);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int launch_pool(const oai_unet* h, const float* in, float* out, const int dims[3], int C, int ntiles, hipStream_t st, int shell_only) {
    if (h->sres) {
        const int nch = (C + 15) / 16;
        const size_t Do = dims[0] / 2, Ho = dims[1] / 2, Wo = dims[2] / 2;
        const size_t faces = Do * Ho * Wo - (Do - 2) * (Ho - 2) * (Wo - 2) - (shell_only == 2 ? 2 * Ho * Wo : 0);
        const size_t total = (size_t)ntiles * (shell_only ? faces : Do * Ho * Wo) * nch * 4;
        maxpool2_sres_kernel<<<capped_blocks(total, 256 * 32), 256, 0, st>>>(reinterpret_cast<const unsigned char*>(in), reinterpret_cast<unsigned char*>(out),
                                                                dims[0], dims[1], dims[2], nch, total, shell_only);
        OAI_CHECK_LAUNCH();
        return OAI_OK;
    }
    const size_t total4 = (size_t)ntiles * (dims[0] / 2) * (dims[1] / 2) * (dims[2] / 2) * (C / 4);
    maxpool2_kernel<<<capped_blocks(total4, 256 * 32), 256, 0, st>>>(in, out, dims[0], dims[1], dims[2], C, total4);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// ec0 (+ gather) of every tile of the batch, where it is not fused into ec1's staging
int launch_first(const oai_unet* h, const TileSource& src, float* e0, int ntiles, hipStream_t st) {
    const Layer* L = h->L;
    const size_t v0 = (size_t)src.td * src.th * src.tw;
    const dim3 grid_all(cdiv(v0 / 2, 256), ntiles);                                          // one workgroup per 256 voxel pairs (the fp32 kernel)
    const dim3 grid(std::min<unsigned>(cdiv(v0 / 2, 256), (unsigned)h->opt_first_blocks), ntiles);     // the split-resident kernel walks the pairs with a grid stride
    const int c = L[EC0].cout;
    unsigned char* e0s = reinterpret_cast<unsigned char*>(e0);
    const bool f16 = h->precision == OAI_PREC_FP16X3;
    const float* sc0 = f16 ? L[EC0].scale_f16 : L[EC0].scale;
    const float* sh0 = f16 ? L[EC0].shift_f16 : L[EC0].shift;
    unsigned* cen0 = census_of(h, EC0);
    if (h->sres && c == 32) conv3_first_sres_kernel<32><<<grid, 256, 0, st>>>(src, L[EC0].plain, sc0, sh0, e0s, 1, h->range_flag, cen0, 0);
    else if (h->sres && c == 16) conv3_first_sres_kernel<16><<<grid, 256, 0, st>>>(src, L[EC0].plain, sc0, sh0, e0s, 1, h->range_flag, cen0, 0);
    else if (h->sres && c == 8) conv3_first_sres_kernel<8><<<grid, 256, 0, st>>>(src, L[EC0].plain, sc0, sh0, e0s, 1, h->range_flag, cen0, 0);
    else if (c == 32) conv3_first_kernel<32><<<grid_all, 256, 0, st>>>(src, L[EC0].plain, sc0, sh0, e0, 1);
    else if (c == 16) conv3_first_kernel<16><<<grid_all, 256, 0, st>>>(src, L[EC0].plain, sc0, sh0, e0, 1);
    else if (c == 8) conv3_first_kernel<8><<<grid_all, 256, 0, st>>>(src, L[EC0].plain, sc0, sh0, e0, 1);
    else return set_error(OAI_ERR_ARG, "ec0 cout %d unsupported (8, 16 or 32)", c);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// shared encoder pass: ec0 where ec1's shell reads it: closer than 3 voxels to a face (voxel pairs along x, enumerated slab by slab); dims = the tile
int launch_first_shell(const oai_unet* h, const TileSource& src, float* e0, const int dims[3], int ntiles, hipStream_t st) {
    const Layer* L = h->L;
    const size_t pairs = (size_t)6 * dims[1] * (dims[2] / 2) + (size_t)(dims[0] - 6) * 6 * (dims[2] / 2) + (size_t)(dims[0] - 6) * (dims[1] - 6) * 4;
    dim3 grid(std::min<unsigned>(cdiv(pairs, 256), (unsigned)h->opt_first_blocks), ntiles);
    conv3_first_sres_kernel<32><<<grid, 256, 0, st>>>(src, L[EC0].plain, L[EC0].scale_f16, L[EC0].shift_f16, reinterpret_cast<unsigned char*>(e0), 1,
                                                      h->range_flag, census_of(h, EC0), 3);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// shared encoder pass: the interior of the batch's pooled tensors is a copy out of the volume-wide one; dims = the pooled tile level
int launch_pooled_gather(const oai_unet* h, const SharedEnc& se, const TileSource& src, float* p0, const int dims[3], int ntiles, hipStream_t st) {
    const int nch1 = (h->L[EC1].cout + 15) / 16;
    const size_t total = (size_t)ntiles * (dims[0] * dims[1] * dims[2]) * nch1 * 4;
    pooled_gather_kernel<<<capped_blocks(total, 256 * 64), 256, 0, st>>>(reinterpret_cast<const unsigned char*>(se.SP0), reinterpret_cast<unsigned char*>(p0), src,
                                                           dims[0], dims[1], dims[2], se.PD / 2, se.PH / 2, se.PW / 2, nch1, total);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// dc0 + sigmoid/threshold + centre crop as a launch of its own: blocks are laid out over the full kept centre `keep`; origin / eff = the kept centre's
// first voxel and extent in the tile's blocks
int launch_head(const oai_unet* h, const float* in, const int dims[3], const Box& keep, const int origin[3], const int eff[3], int out_mode,
                float* blocks_out, const int* boxes, int ntiles, hipStream_t st) {
    const Layer* L = h->L;
    const Box& k = keep;
    const float* hw = h->precision == OAI_PREC_FP16X3 ? L[DC0].plain_f16 : L[DC0].plain;
    const int bz = k.hi[0] - k.lo[0], by = k.hi[1] - k.lo[1], bx = k.hi[2] - k.lo[2];
    dim3 grid(cdiv((size_t)bz * by * bx, 256), ntiles);
    if (h->sres)
        head_sres_kernel<<<grid, 256, 0, st>>>(reinterpret_cast<const unsigned char*>(in), L[DC0].cin, dims[0], dims[1], dims[2],
                                               k.lo[0], k.lo[1], k.lo[2], bz, by, bx, origin[0], origin[1], origin[2], eff[0], eff[1], eff[2], hw,
                                               L[DC0].shift, h->n_classes, out_mode, blocks_out, boxes);
    else
    head_kernel<<<grid, 256, 0, st>>>(in, L[DC0].cin, dims[0], dims[1], dims[2], k.lo[0], k.lo[1], k.lo[2],
                                      bz, by, bx, origin[0], origin[1], origin[2], eff[0], eff[1], eff[2], hw, L[DC0].shift, h->n_classes,
                                      out_mode, blocks_out, boxes);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

// Lower edge of the calibrated range: a layer whose largest stored activation is below kLowRange (and not zero) is at least 128 x smaller
// than at calibration time (or was never calibrated): its low split terms are subnormal and the result is no longer fp32 grade.
constexpr float kLowRange = 8.0f;

// dst[0] = range flag of the work queued so far: bit 0 = an activation beyond fp16's range (set by the kernels), bit 1 = a layer's
// maximum below kLowRange (from the census).  One wave; `reset` clears the flag and the census for the next volume.
__global__ void range_eval_kernel(int* __restrict__ flag, unsigned* __restrict__ census, int* __restrict__ dst, int reset, float low) {
    const int t = threadIdx.x;
    unsigned m = 0;
    if (t < 18)
        for (int i = 0; i < 16; ++i) m = max(m, census[t * 16 + i]);
    const bool lowhit = t < 17 && m != 0 && __uint_as_float(m) < low;
    const unsigned long long any = __ballot(lowhit);
    if (t == 0) {
        dst[0] = flag[0] | (any ? 2 : 0);
        if (reset) flag[0] = 0;
    }
    if (reset && t < 18)
        for (int i = 0; i < 16; ++i) census[t * 16 + i] = 0;
}

// the raw form of range_eval_kernel: [0] = overflow bit, [1 + k] = layer k's maximum (float bits); clears flag and census
__global__ void range_state_kernel(int* __restrict__ flag, unsigned* __restrict__ census, int* __restrict__ dst) {
    const int t = threadIdx.x;
    if (t < 18) {
        unsigned m = 0;
        for (int i = 0; i < 16; ++i) { m = max(m, census[t * 16 + i]); census[t * 16 + i] = 0; }
        dst[1 + t] = (int)m;
    }
    if (t == 0) { dst[0] = flag[0] & 1; flag[0] = 0; }
}

__global__ void range_flag_from_state_kernel(const int* __restrict__ state, int* __restrict__ dst, float low) {
    const int t = threadIdx.x;
    const unsigned m = t < 17 ? (unsigned)state[1 + t] : 0u;
    const bool lowhit = t < 17 && m != 0 && __uint_as_float(m) < low;
    const unsigned long long any = __ballot(lowhit);
    if (t == 0) dst[0] = (state[0] & 1) | (any ? 2 : 0);
}

int launch_range_eval(const oai_unet* h, int* dst, int reset, hipStream_t st) {
    range_eval_kernel<<<1, 64, 0, st>>>(h->range_flag, h->census, dst, reset, kLowRange);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}
int launch_range_state(const oai_unet* h, int* dst, hipStream_t st) {
    range_state_kernel<<<1, 64, 0, st>>>(h->range_flag, h->census, dst);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}
int launch_range_flag_from_state(const int* state, int* dst, hipStream_t st) {
    range_flag_from_state_kernel<<<1, 64, 0, st>>>(state, dst, kLowRange);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

int stitch_impl(const float* blocks, int ncls, int D, int H, int W, const int tile[3], const int overlap[3],
                const int crop[3], float* maps, void* stream, const StitchRanges& rg) {
    OAI_CHECK_ARG(blocks && maps && tile && overlap, "oai_stitch_blocks: null pointer");
    int eff[3], grid[3];
    const int size[3] = {D, H, W};
    for (int i = 0; i < 3; ++i) {
        eff[i] = tile[i] - 2 * overlap[i];
        OAI_CHECK_ARG(eff[i] > 0, "oai_stitch_blocks: overlap too large for the tile");
        grid[i] = (size[i] + eff[i] - 1) / eff[i];
    }
    const size_t total = (size_t)ncls * D * H * W;
    if (crop && (crop[0] == 0 || crop[1] == 0 || crop[2] == 0)) {
        // image_transforms.py:509-513 copies [c:-c] per axis into a zero array; with c == 0 the numpy slice 0:-0 is EMPTY, so a
        // crop_size with a zero component (an overlap of 0 on some axis) yields an all-zero map in the reference.  Reproduced.
        OAI_CHECK_HIP(hipMemsetAsync(maps, 0, total * sizeof(float), (hipStream_t)stream));
        return OAI_OK;
    }
    stitch_kernel<<<capped_blocks(total, 256 * 32), 256, 0, (hipStream_t)stream>>>(blocks, ncls, D, H, W, eff[0], eff[1], eff[2], grid[1], grid[2],
                                                                crop ? crop[0] : 0, crop ? crop[1] : 0, crop ? crop[2] : 0, maps, rg);
    OAI_CHECK_LAUNCH();
    return OAI_OK;
}

}  // namespace oai
