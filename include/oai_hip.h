/* liboai_hip.so -- C ABI of the MI355X (gfx950) hot path of OAI_analysis_2.
 *
 * The reference (uncbiag/OAI_analysis_2 @ 2024_10_08) has no FFI of its own: its seam is
 * Python duck typing.  The entry points below are what a binding for that seam
 * calls; each one names the reference interface it stands in for.  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; oai_last_error() gives the text
 *     (thread-local).  Nothing aborts, nothing throws across the boundary.
 *   - every pointer named *_dev is device memory owned by the caller (e.g. a PyTorch-ROCm
 *     tensor's data_ptr()); host pointers are named *_host.  No torch types cross the boundary.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Launch functions
 *     enqueue work and return; they never synchronise, allocate or free (graph-capturable).
 *   - volumes are [z][y][x] (numpy / torch order), fp32 unless stated.  Vector fields and
 *     coordinate maps are channel-first [3][D][H][W], channel c along tensor axis c (z,y,x),
 *     in ICON's normalised [0,1] units (index / (n-1)).
 *   - a handle is not thread-safe; distinct handles are.
 */
#ifndef OAI_HIP_H
#define OAI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OAI_OK 0
#define OAI_ERR_ARG 1
#define OAI_ERR_HIP 2
#define OAI_ERR_WORKSPACE 3

int oai_version(void);
const char* oai_last_error(void);
/* Fills name (<= cap bytes) with the device's gcnArchName; returns the CU count or -1. */
int oai_device_info(char* name, int cap);

/* ------------------------------------------------------------------------------------------
 * Registration warp family.  Replaces torch.nn.functional.grid_sample / avg_pool3d /
 * interpolate as reached from oai_analysis/registration.py:25 (icon_registration.itk_wrapper.
 * register_pair -> network_wrappers / mermaidlite.compute_warped_image_multiNC), and the ITK
 * resample of test/test_all.py:42-52 / oai_analysis/dask_processing.py:95-111.
 * ---------------------------------------------------------------------------------------- */

/* out[c][D][H][W] = trilinear sample of src[c][d][h][w] at coords (ICON [0,1] units; border
 * clamp, align_corners=True).  coords_dev == NULL means the identity map of [D][H][W].
 * = mermaidlite.compute_warped_image_multiNC(src, coords, spacing, 1). */
int oai_grid_sample3d(const float* src_dev, int C, int d, int h, int w,
                      const float* coords_dev, int D, int H, int W, float* out_dev, void* stream);

/* Process-wide tuning options of the warp kernels (bit-preserving; the library does not read the environment):
 *   "brick" 0|1 (0)  oai_grid_sample3d / oai_compose (C = 1 or 3) through sample_brick_kernel: a block owns a 16 x 8 x 4 output brick and, when the
 *                    bounding box of the brick's corners fits 24 KB, stages that box of the source in LDS by LDS-DMA and takes the corners
 *                    from there (the gather form is bound by the CU's L1 tag pipeline: profiles/r02_registration.md); bricks whose box does
 *                    not fit gather from memory as before.  Same arithmetic in the same order: bit-identical outputs.  Replaces the same
 *                    reference op, mermaidlite.compute_warped_image_multiNC as reached from oai_analysis/registration.py:25. */
int oai_warp_set_option(const char* name, int value);

/* out = coords + sample(disp, coords): FunctionFromVectorField's transform(coords).
 * coords_dev == NULL means the identity map (the "sampled" path at another resolution);
 * if additionally (d,h,w)==(D,H,W) and shortcut != 0, out = identity + disp exactly
 * (the package's isIdentity shortcut, no interpolation). */
int oai_compose(const float* disp_dev, int d, int h, int w, const float* coords_dev,
                int D, int H, int W, int shortcut, float* out_dev, void* stream);

/* F.avg_pool3d(x, 2, ceil_mode=True) on [C][D][H][W] -> [C][ceil(D/2)][ceil(H/2)][ceil(W/2)]. */
int oai_avgpool2_3d(const float* in_dev, int C, int D, int H, int W, float* out_dev, void* stream);

/* F.interpolate(x, size=(D,H,W), mode="trilinear", align_corners=False) on [C][d][h][w]. */
int oai_resize_trilinear(const float* in_dev, int C, int d, int h, int w,
                         float* out_dev, int D, int H, int W, void* stream);

/* itk_wrapper.create_itk_transform's vector image: disp[z][y][x][3] (float64, components x,y,z,
 * network-voxel units) = reverse_components((phi - identity) * (shape - 1)). */
int oai_phi_to_itk_displacement(const float* phi_dev, int D, int H, int W, double* disp_dev, void* stream);

/* A whole compose chain of icon_registration's TwoStepRegistration / DownsampleRegistration closures per output voxel, without
 * materialising the intermediate maps (SURVEY.md K15 "fuse chains", K18):
 *     c = identity(D,H,W) [+ start_dev]        start_dev [3][D][H][W] may be NULL (the package's isIdentity shortcut when given)
 *     c = c + sample(fields[i], c)             i = 0 .. n_fields-1 (n_fields <= OAI_WARP_CHAIN_MAX_FIELDS), fields[i] is
 *                                              [3][fd][fh][fw] with (fd,fh,fw) = field_dims_zyx[3i..3i+2] -- any resolution; a step
 *                                              tree of N FunctionFromVectorFields flattens to N links (oai_icon_create)
 *     out = image_dev ? sample(image_dev [id][ih][iw], c)  ->  out_dev [D][H][W]
 *                     : c                                   ->  out_dev [3][D][H][W]
 * `sample` is oai_grid_sample3d's (grid_sample bilinear / border / align_corners=True on [0,1] coordinates).  Bit-identical to
 * the sequence of oai_compose / oai_grid_sample3d calls it replaces.  `fields` and `field_dims_zyx` are HOST arrays. */
#define OAI_WARP_CHAIN_MAX_FIELDS 8
int oai_warp_chain(const float* start_dev, int D, int H, int W, int n_fields, const float* const* fields,
                   const int* field_dims_zyx, const float* image_dev, int id, int ih, int iw, float* out_dev, void* stream);

/* Geometry of one image for the resample: index_xyz -> physical = A*idx + b (row-major 3x3 + 3). */
typedef struct oai_affine { double A[9]; double b[3]; } oai_affine;

/* warped[zB][yB][xB] = prob_A(phi_AB(p)): ITK ResampleImageFilter(prob, transform=phi_AB,
 * LinearInterpolateImageFunction, reference grid = image_B, default pixel 0), with phi_AB the
 * CompositeTransform [to_network_space, DisplacementFieldTransform, from_network_space].
 *   b_index_to_net : B index  -> network index space   (T_B^-1 o index_to_physical_B)
 *   net_to_a_index : network index space -> A continuous index (physical_to_index_A o T_A)
 *   disp_dev       : float64 [Dn][Hn][Wn][3] from oai_phi_to_itk_displacement. */
int oai_resample_through_disp(const float* prob_dev, int nzA, int nyA, int nxA,
                              const double* disp_dev, int Dn, int Hn, int Wn,
                              const oai_affine* b_index_to_net, const oai_affine* net_to_a_index,
                              float* out_dev, int nzB, int nyB, int nxB, void* stream);

/* The same resample for n_maps (1..4) probability maps probs_dev[n_maps][nzA][nyA][nxA] at once, straight from the network's
 * dense map phi_dev[3][Dn][Hn][Wn] (fp32, [0,1] units): create_itk_transform's displacement (fp32 arithmetic, widened to
 * double -- the value oai_phi_to_itk_displacement stores) is rebuilt at the 8 corners in registers, so neither the 71 MB
 * fp64 field nor a second pass over phi exists.  Results are bit-identical to oai_phi_to_itk_displacement +
 * oai_resample_through_disp per map.  Replaces the two deform_probmap calls of test/test_all.py:54-58 /
 * dask_processing.py:95-111.  out_dev[n_maps][nzB][nyB][nxB].  nxA >= 2 (the two x corners of a row are one 8-byte gather). */
int oai_resample_maps_through_phi(const float* probs_dev, int n_maps, int nzA, int nyA, int nxA,
                                  const float* phi_dev, int Dn, int Hn, int Wn,
                                  const oai_affine* b_index_to_net, const oai_affine* net_to_a_index,
                                  float* out_dev, int nzB, int nyB, int nxB, void* stream);

/* ------------------------------------------------------------------------------------------
 * Intensity windowing, the step just before the hot path: image_normalize(image, lo, hi, omin, omax) of
 * oai_analysis/dask_processing.py:10-26 (called with 0.1, 99.9, 0, 1 at :75 and :177) =
 * np.percentile window (exact order statistics, numpy float32 interpolation) + itk.IntensityWindowingImageFilter.
 * window_out_dev (optional, 2 floats on the device) receives (window_min, window_max).
 * ---------------------------------------------------------------------------------------- */
size_t oai_image_normalize_workspace_bytes(void);
int oai_image_normalize(const float* in_dev, size_t n, float pct_lo, float pct_hi, float out_min, float out_max,
                        float* out_dev, float* window_out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation.  Replaces `self.model(temp_input.to(self.device)).cpu()` and the code around
 * it in Segmenter3DInPatchClassWise.segment (oai_analysis/segmentation/segmenter.py:100-131):
 * Partition.__call__ (image_transforms.py:395-455), UNet.forward (networks.py:109-149),
 * torch.sigmoid / >0.5 (segmenter.py:121-124) and Partition.assemble (image_transforms.py:457-519).
 * ---------------------------------------------------------------------------------------- */

typedef struct oai_unet oai_unet;

/* One conv block in the reference's own tensor layouts (host memory, fp32):
 *   kind 0: Conv3d k3 s1 p1           weight [Cout][Cin][3][3][3]
 *   kind 1: ConvTranspose3d k3 s1 p1  weight [Cin][Cout][3][3][3]
 *   kind 2: ConvTranspose3d k2 s2     weight [Cin][Cout][2][2][2]
 *   kind 3: Conv3d k1                 weight [Cout][Cin]
 * bias / bn_* may be NULL (bias=False / BN=False, networks.py:39). */
typedef struct oai_layer_params {
    int kind, cin, cout;
    const float* weight_host;
    const float* bias_host;
    const float* bn_gamma_host;
    const float* bn_beta_host;
    const float* bn_mean_host;
    const float* bn_var_host;
} oai_layer_params;

#define OAI_UNET_NUM_LAYERS 18 /* ec0..ec7, dc9, dc8, dc7, dc6, dc5, dc4, dc3, dc2, dc1, dc0 */

/* Ingests a reference state_dict (strict, like utils.initialize_model, utils.py:29): packs
 * the weights for the kernels (transposed-conv flip, K-permuted MFMA panels) and uploads them. */
int oai_unet_create(const oai_layer_params layers_host[OAI_UNET_NUM_LAYERS], float bn_eps, oai_unet** out);
void oai_unet_destroy(oai_unet* h);

/* Arithmetic of the 3x3x3 conv layers and the k2s2 up-convs (ec0, the head and everything outside the U-Net are always fp32).  A handle
 * starts in OAI_PREC_F32; the Python surface (Segmenter3DInPatchClassWise, bench.py) selects OAI_PREC_FP16X3 by default and falls back to
 * OAI_PREC_F32 per volume when the range flag is raised:
 *   OAI_PREC_F32     v_mfma_f32_32x32x2_f32: exact fp32 products; the accumulation is TWO-LEVEL (round 5): one fresh accumulator set per
 *                    8-channel chunk (108 MFMAs), folded into the running sum by one fp32 add -- 0.8 x the reference's own distance from its
 *                    float64 run on four reference networks (one running sum over K = 27 Cin: 2.9-3.5 x).  Activations fp32 in memory.
 *   OAI_PREC_BF16X6  every fp32 operand split into 3 bf16 terms, 6 bf16 MFMA passes per product: fp32-grade
 *                    results (dropped terms are O(2^-24)) at 2.7x the fp32 MFMA rate.  Activations fp32 in memory, split while staging.
 *   OAI_PREC_BF16X3  2 terms, 3 passes: ~2^-17 relative error per product, 5.3x the fp32 MFMA rate.  Activations fp32 in memory.
 *   OAI_PREC_FP16X3  (below) activations live in memory AS their two fp16 terms ("format S", 4 bytes per element like fp32: unet_sres.h),
 *                    scaled per layer by a power of two (oai_unet_calibrate_step); fp32 in and out of every entry point.
 * Collectives: there is no oai_comm_* / oai_zslab_* entry point (SURVEY.md 8b lists them as candidates) BY DESIGN -- the multi-GPU
 * exchange steps (volume broadcast, all_gather of kept-centre blocks, z-slab gather, the 76-byte range state) are torch.distributed
 * calls over RCCL on device tensors in oai_analysis_2_amd/parallel.py: host orchestration stays in Python (BASELINE.json north_star),
 * and this library only provides what those steps need on either side (oai_segment_tiles' tile ranges, oai_stitch_blocks_ranged,
 * oai_resample_maps_through_phi's z ranges, oai_unet_range_state_snapshot). */
#define OAI_PREC_F32 0
#define OAI_PREC_BF16X3 1
#define OAI_PREC_BF16X6 2
#define OAI_PREC_FP16X3 3 /* 2 fp16 terms (22 mantissa bits), 3 fp16 MFMA passes: fp32-grade results at the BF16X3 rate; needs
                             activations below 65504 in magnitude (weights are range-scaled per output channel, exactly) */
int oai_unet_set_precision(oai_unet* h, int mode);
/* OAI_PREC_FP16X3 only: *out = the range flag of the work queued since the last reset; non-zero means the results of that
 * run are invalid and it must be repeated with OAI_PREC_F32 (what Segmenter3DInPatchClassWise / VolumePipeline do):
 *   bit 0  an activation was beyond fp16's range (|x| * 2^e > 65504);
 *   bit 1  some layer's largest stored activation was below 8.0 (and not zero): its low fp16 terms are subnormal, the
 *          arithmetic is no longer fp32 grade.  Either the handle was never calibrated or this input is > 128 x quieter
 *          than the calibration input (oai_unet_calibrate_step).
 * A network replaces nothing in the reference here: segmenter.py:52-62 loads an arbitrary checkpoint whose per-layer
 * activation scale is free, and networks.py:109-149 runs it in fp32, which has no such window.
 * The read (and the reset) are ordered on `stream` -- pass the stream the segment calls were queued on -- and the call
 * blocks until that stream has drained. */
int oai_unet_range_flag(oai_unet* h, int reset, int* out, void* stream);
/* Asynchronous form for pipelined callers (cohort.py): evaluates the flag word into dst_dev[0] and clears flag and census,
 * queued on `stream` behind the segment calls of ONE volume, so the flag is attributed to that volume; the caller reads
 * dst_dev with its own D2H copy of the results.  No synchronisation. */
int oai_unet_range_flag_snapshot(oai_unet* h, int* dst_dev, void* stream);
/* The same snapshot as RAW STATE for a volume whose tiles were computed by several ranks (pipeline.run_sharded): state_dev[0] = the
 * overflow bit, state_dev[1 + k] = the bits of layer k's largest stored activation (a non-negative float: ordered like its integer
 * bits), so that an elementwise MAX all-reduce over the ranks gives the state of the WHOLE volume -- a rank that holds only quiet
 * background tiles must not raise the LOW bit on its own subset.  Clears flag and census like the snapshot.
 * oai_unet_range_flag_from_state evaluates a (reduced) state into the two-bit flag word, flag_dev[0]. */
#define OAI_UNET_RANGE_STATE_WORDS (1 + OAI_UNET_NUM_LAYERS)
int oai_unet_range_state_snapshot(oai_unet* h, int* state_dev, void* stream);
int oai_unet_range_flag_from_state(const int* state_dev, int* flag_dev, void* stream);
/* Per-layer activation exponents of OAI_PREC_FP16X3.  Layer k (order of OAI_UNET_NUM_LAYERS) stores its output as
 * x * 2^e[k] in fp16 term pairs; powers of two fold exactly into the epilogue affine of the producer, the epilogue scale of
 * the consumer and -- for the skip inputs of dc8 / dc5 / dc2 -- the weight panel, so results change only where fp16's
 * exponent range had been costing bits.  e[17] (dc0: logits) is always 0.
 *   oai_unet_census          max |stored activation| per layer since the last reset (0 = nothing stored); blocks on `stream`.
 *   oai_unet_calibrate_step  call after one oai_segment_tiles / oai_unet_forward_tiles pass over representative input:
 *                            moves every layer whose maximum is outside [2^9, 2^12) to [2^10, 2^11), resets census and flag,
 *                            *more = 1 if anything moved (run another pass and call again; a layer downstream of an overflow
 *                            is only right after its inputs are), 0 = calibrated.  Two passes for a healthy network.
 *   oai_unet_set_act_exponents / get  explicit form (reproducible runs, all ranks of a tile-sharded volume).  Set waits for
 *                            the device (hipDeviceSynchronize) and rewrites the handle's epilogue arrays in place. */
int oai_unet_census(oai_unet* h, float max_out[OAI_UNET_NUM_LAYERS], int reset, void* stream);
int oai_unet_calibrate_step(oai_unet* h, void* stream, int* more);
int oai_unet_get_act_exponents(const oai_unet* h, int e_out[OAI_UNET_NUM_LAYERS], int* calibrated);
int oai_unet_set_act_exponents(oai_unet* h, const int e[OAI_UNET_NUM_LAYERS]);
/* Tuning options of the OAI_PREC_FP16X3 path (bit-preserving -- same k order, identical maps -- except "winograd" / "winograd_layers" / "m16" / "m16_layers"), by name
 * (the library does not read the environment):
 *   "sres" 0|1 (1)      activations resident as fp16 term pairs (unet_sres.h) / fp32-resident split kernels
 *   "sres_mrep" 2|4 (4) z slices per workgroup of the split-resident conv kernel
 *   "xcd_group" n (32)  logical blocks dealt to one XCD at a time; 0 = plain launch order
 *   "fuse_first" 0|1 (1) ec0 (networks.py:43) computed inside ec1's halo staging instead of as its own launch (when ec1 is one main-shape launch)
 *   "wide" 0|1|2 (1)    layers with Cout % 128 == 0 run conv3_igemm_sres2: one 8-wave workgroup per CU computes 128 couts of a
 *                       block from ONE double-buffered halo box (unet_sres2.h); 1 = launches of >= 1024 workgroups, 2 = always
 *   "shared_enc" 0|1 (1) oai_segment_tiles computes ec0 -> ec1 once over the padded volume + a 2-voxel shell per tile (needs the workspace
 *                       of oai_segment_workspace_bytes; geometries it does not fit fall back to per-tile computation)
 *   "winograd" 0..63 (19) NOT bit-preserving (same precision class, other rounding points; probabilities within ~2e-6 of the direct
 *                       form's): the plain k3 layers (no fused ec0 / pool / head) run conv3_wino_sres (unet_wino.h), the x axis in Winograd
 *                       F(2,3) form = 2/3 of the MFMAs.  bit 0: layers with Cout % 128 == 0, bit 1: layers with one block of 64 couts
 *                       and >= 8 input chunks (dc2); 0 = the direct kernels everywhere; bits 2, 3: A/B of alternative kernel forms; bit 4 (round 4): the
 *                       two-group form's taps on v_mfma_f32_16x16x32_f16 with K = a pair of taps (same cycles per FLOP, the shape the chip clocks
 *                       ~13 % higher at the power wall; another summation order, same gates); bit 5: the same for the 64-cout layer, all its launch shapes
 *                       (measured within noise of bit 4 alone: not in the default).  A value depends on the parity of its voxel's x only -- not on blocks, strips
 *                       or batching.  "winograd_layers" (mask, all): bit k = layer k may take it (A/B of single layers)
 *   "m16" 0|1 (1)       NOT bit-preserving (round 5): the direct kernel conv3_igemm_sres -- ec1 with the fused ec0, ec2, dc1 with the fused head, and any
 *                       layer "winograd" leaves to it -- runs its taps on v_mfma_f32_16x16x32_f16 with K = a PAIR of taps (27 = 13 pairs + 1) for every
 *                       layer with Cout % 128 != 0 (a layer that may take the bit-identical 128-cout form conv3_igemm_sres2 keeps 32x32x16, so "wide"
 *                       stays bit-preserving); every launch shape of the kernel has the variant: one summation order per layer.  Same cycles per FLOP,
 *                       +12-14 % clock at the power wall: ec1 16.8 -> 14.6, ec2 4.9 -> 3.9, dc1 8.5 -> 7.2 ms per 160 tiles.  "m16_layers" (mask, all):
 *                       bit k = layer k may take it (A/B of single layers)
 *   "winograd_f32" 0|1 (1) NOT bit-preserving (round 6): every k3 layer of OAI_PREC_F32 (ec1 ... dc1; ec1 / ec3 / ec5 with their MaxPool3d fused where the launch is a
 *                       whole tile) runs conv3_wino_f32 (unet_wino_f32.h): the x axis in Winograd F(2,3) form, exact fp32 products, the direct kernel's two-level
 *                       accumulation = 2/3 of the fp32 MFMAs (pass 590 -> 445 ms), and 0.66-0.70 x the reference's own fp32 distance from its float64 run where the
 *                       direct form (0) sits at 0.80-0.83 (profiles/r06_wino_f32.md).  A voxel's bits depend on the parity of its x, not on batches, launch boxes or
 *                       strips.  "winograd_layers" applies
 *   "first_blocks" 1..4096 (24) bit-preserving (round 6): workgroups per tile of the ec0 kernel (networks.py:43 where it is not fused into ec1's staging: the 3-voxel
 *                       shell of every tile, the fp16x3 path without fuse_first); each walks the tile's voxel pairs with a grid stride, the next pair's 36 inputs
 *                       gathered under the current pair's FMAs (2.17 -> 1.38 ms per 160 tiles)
 *   "up_nbw" 0..64 (0)  bit-preserving (round 6): column blocks of 256 a workgroup of the k2s2 up-conv kernel (networks.py:56,59,62) walks one after the other over its
 *                       128 voxels -- the voxel table, the A-row plan and the workgroup launch are paid once per walk; 0 = as many as keep >= 16 workgroups per slot of
 *                       the chip, 1 = one column block per workgroup (rounds 1-5), n = at most n
 *   "own_cover" 0|1 (1) bit-preserving: in oai_segment_tiles the trimmed decoder convs (dc8, dc7, dc5, dc4, dc2 on the Winograd kernel) place their blocks on every tile's
 *                       OWN cover -- origin at the tile's own box corner (x rounded down to even), strips decided by its own remainders, one launch per block shape --
 *                       and the k2s2 up-convs list the voxels of every tile's own input box; 0 = the cover / the voxels of the batch's union box (border tiles
 *                       then pay for blocks that straddle the union's grid and for rows outside their box).  oai_unet_cover_stats counts both
 *   "one_launch" 0..7 (1) bit-preserving: an own-cover layer runs as ONE launch over a device list of the batch's live blocks -- all main blocks, then the x strips,
 *                       then the y strips, so that the strips fill the main blocks' last round and the layer pays one tail instead of three (conv3_wino_list*,
 *                       csrc/unet_wino.h; the blocks run the stand-alone kernels' own code).  bit 0: the layers with two cout groups (dc8, dc7, dc5, dc4), bit 1: the
 *                       64-cout layer (dc2; not in the default: merged with its strips the specialised form spills more registers inside its chunk loop,
 *                       profiles/one_launch.md), bit 2: force.  There is a SIZE GATE: without bit 2 a layer is merged only in a batch where its live blocks number
 *                       at least the device's CUs.  Smaller batches keep the three launches: they have no tail worth saving, their launch structure is pinned by the
 *                       tests, and they are not what the library is timed on.  0 = three launches per layer.  Needs "own_cover"; oai_unet_block_list gives the list
 *   "dead_stores" 0|1 (1) the encoder does not write the part of a skip tensor that the trimmed decoder never reads
 *   "census" 0|1 (1)    the kernels record per-layer activation maxima (activation exponents, LOW bit of the range flag)
 *   "calibrated" 0      forget that the activation exponents were calibrated (they keep their values): oai_unet_get_act_exponents reports 0 until
 *                       oai_unet_set_act_exponents or a settled oai_unet_calibrate_step.  For a caller that found its calibration unfit for the data
 *                       (three flagged volumes in a row under a sidecar file): ONE place holds "calibrated?" -- this handle.  Only 0 is accepted
 * Unknown names and out-of-range values return OAI_ERR_ARG. */
int oai_unet_set_option(oai_unet* h, const char* name, int value);

/* Bytes of device scratch oai_unet_forward_* needs for `batch` tiles of (td,th,tw). */
size_t oai_unet_workspace_bytes(const oai_unet* h, int td, int th, int tw, int batch);
/* ... and what oai_segment_tiles would like for a (D,H,W) volume: the same plus the max-pooled ec1 over the reflect-padded volume (1 GB at
 * 384x384x160) when the geometry allows the shared encoder pass -- ec0 -> ec1 (networks.py:109-113) computed once per volume instead of once
 * per overlapping tile (image_transforms.py:407-434: tiles overlap 2 x 1.33 x 1.33), bit-identical maps.  With only
 * oai_unet_workspace_bytes the call computes every tile on its own. */
size_t oai_segment_workspace_bytes(const oai_unet* h, int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3], int batch);

/* B3 seam: logits[B][n_classes][td][th][tw] = UNet(tiles[B][1][td][th][tw]) (NCDHW like
 * networks.py:109-149), zero conv padding at the tile border, no trimming. */
int oai_unet_forward_tiles(oai_unet* h, const float* tiles_dev, float* logits_dev, int B,
                           int td, int th, int tw, void* workspace_dev, size_t workspace_bytes,
                           void* stream);

/* Fused a3-a7 of SURVEY.md 8a for tiles [tile_begin, tile_end) of the reference's z-major tile
 * order: reflect-pad addressing of vol[D][H][W] (no tiles materialised) -> UNet on each tile ->
 * 1x1x1 head -> sigmoid (out_mode 0) or sigmoid>0.5 as 0/1 (out_mode 1) or raw logits (2) ->
 * kept centre blocks blocks_dev[tile - tile_begin][n_classes][ez][ey][ex] (e = tile - 2*overlap).
 * Only what the stitched result can depend on is computed (bit-identical dead-output trim): per layer the
 * box its consumers need, and per tile only the part of the kept centre that
 * Partition.assemble keeps -- crop_zyx (may be NULL) is the frame oai_stitch_blocks will zero, and the part
 * beyond the image is trimmed.  Block voxels outside that part are left unwritten. */
int oai_segment_tiles(oai_unet* h, const float* vol_dev, int D, int H, int W,
                      const int tile_zyx[3], const int overlap_zyx[3], const int crop_zyx[3],
                      int tile_begin, int tile_end,
                      int out_mode, float* blocks_dev, int batch,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* Partition.assemble (non-vote branch): scatter centre blocks of ALL tiles into
 * maps[n_classes][D][H][W], trim to the image, zero the outer frame of crop_zyx voxels.  A crop with a zero component
 * gives an all-zero map, as the reference's `[c:-c]` slicing does (image_transforms.py:509-513). */
int oai_stitch_blocks(const float* blocks_dev, int n_classes, int D, int H, int W,
                      const int tile_zyx[3], const int overlap_zyx[3], const int crop_zyx[3],
                      float* maps_dev, void* stream);

/* The same assemble, reading the blocks where an all_gather of per-rank tile ranges left them (the reference's
 * counterpart is the Dask gather of per-task results, dask_processing.py:170-189): rank r computed the tiles
 * [bounds_host[r], bounds_host[r + 1]) and its blocks sit in slots [r * slot_stride, r * slot_stride + its count) of blocks_dev --
 * ragged ranges are padded to slot_stride blocks per rank by the collective (all_gather_into_tensor needs equal pieces), and this
 * entry reads through the table instead of a compacting copy of 189 MB per volume.  bounds_host: n_ranges + 1 ascending tile
 * indices, [0] = 0, [n_ranges] = the tile count; n_ranges <= 64. */
int oai_stitch_blocks_ranged(const float* blocks_dev, int n_classes, int D, int H, int W,
                             const int tile_zyx[3], const int overlap_zyx[3], const int crop_zyx[3],
                             const int* bounds_host, int n_ranges, int slot_stride,
                             float* maps_dev, void* stream);

/* Partition.__call__ (image_transforms.py:395-455) as a standalone gather: tiles [tile_begin, tile_end) of the reference's
 * z-major order, tiles_dev[t - tile_begin][tz][ty][tx] = reflect-padded volume (pad lo = overlap; numpy.pad 'reflect').  For
 * callers that use Partition directly; oai_segment_tiles never materialises tiles. */
int oai_partition_tiles(const float* vol_dev, int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3],
                        int tile_begin, int tile_end, float* tiles_dev, void* stream);

/* Partition.assemble(is_vote=True) (image_transforms.py:466-484): every tile votes with all its voxels (overlaps included);
 * out_dev[D][H][W] (uint8) = index of the label plane with the most votes (lowest index on a tie, np.argmax).  tile_labels_dev
 * [n_tiles][tz][ty][tx] int32 must hold values in [0, n_labels) -- the reference indexes its vote array with the label VALUE,
 * so its labels are 0..L-1 too. */
int oai_assemble_vote(const int* tile_labels_dev, int n_labels, int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3],
                      unsigned char* out_dev, void* stream);

/* Roofline instrumentation (bench.py): when enabled, every launch of the dominant kernel (the 3x3x3
 * implicit-GEMM conv) is bracketed by hipEvents on the launch stream.  oai_unet_profile_read waits for the
 * recorded events and returns their summed duration and launch count, then clears them. */
int oai_unet_profile(oai_unet* h, int enable);
int oai_unet_profile_read(oai_unet* h, double* conv3_ms, long long* conv3_launches);

/* Algorithmic FLOPs (2*MACs) of one tile, full or with the dead-output trim. */
double oai_unet_tile_flops(const oai_unet* h, int td, int th, int tw, const int overlap_zyx[3], int trimmed);
/* Algorithmic FLOPs of segmenting a whole D x H x W volume as oai_segment_tiles does it (per-tile boxes included);
 * conv3_only restricts the sum to the layers of the 3x3x3 implicit-GEMM kernel. */
double oai_unet_volume_flops(const oai_unet* h, int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3],
                             const int crop_zyx[3], int trimmed, int conv3_only);
/* FLOPs of every tile of a volume as oai_segment_tiles computes it (border tiles cost less: trimmed kept centres): the weights
 * for splitting ONE volume's tiles over ranks (the reference's z-major order; oai_analysis_2_amd/parallel.py). */
int oai_unet_tile_costs(const oai_unet* h, int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3],
                        const int crop_zyx[3], double* costs_host, int n_tiles);
/* Host only, no device and no handle: what option "own_cover" changes for one layer of a volume segmented in batches of `batch` tiles.  `layer` is the
 * schedule index of an own-cover conv layer (dc8 = 9, dc7 = 10, dc5 = 12, dc4 = 13, dc2 = 15) or of an up-conv (dc9 = 8, dc6 = 11, dc3 = 14).
 * stats_host[0] = voxels the tiles need (up-convs: input voxels), [1] = executed with the union's placement (own_cover 0), [2] = executed with every tile's own
 * cover (own_cover 1): a started conv block counts its live z slices x its y x x extent, a started up-conv workgroup its 128 rows.  Counted with the
 * functions the launcher and the device table use.  pieces_host (optional, [n_tiles][4][6] ints, n_tiles = the volume's tile count): per tile the box
 * (lo z y x, hi z y x) and the three pieces of its own cover -- main blocks, x strip, y strip; an up-conv's box is its one piece. */
int oai_unet_cover_stats(int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3], const int crop_zyx[3], int batch, int layer,
                         double stats_host[3], int* pieces_host, int n_tiles);
/* Host only, no device and no handle: the live-block list of option "one_launch" for own-cover conv layer `layer` (indices as above) and the batch of `n` tiles
 * starting at tile_begin, as oai_segment_tiles builds it on the device when it segments the volume in batches of `batch` (n <= batch).  *n_entries = its length
 * (0: the batch does not fit the entry format and keeps its three launches); entries_host (optional, room for `capacity` words) = the entries in list order,
 * one word each: tile index in the batch << 20 | shape << 18 | bz << 12 | by << 6 | bx, shape 0 = main block (4 x 8 x 8), 1 = x strip (4 x 16 x 4), 2 = y strip
 * (4 x 4 x 16), (bz, by, bx) counted from the corner of that piece of the tile's own cover (oai_unet_cover_stats: pieces_host).  workspace_offset (optional): the
 * byte offset in oai_segment_tiles' workspace at which that call leaves the layer's device list of its LAST batch (tests compare the two). */
int oai_unet_block_list(int D, int H, int W, const int tile_zyx[3], const int overlap_zyx[3], const int crop_zyx[3], int batch, int tile_begin, int n, int layer,
                        unsigned* entries_host, int capacity, int* n_entries, long long* workspace_offset);
/* Same as oai_unet_tile_flops, restricted to the layers the 3x3x3 implicit-GEMM kernel runs (ec1-ec7, dc8, dc7, dc5, dc4, dc2, dc1). */
double oai_unet_tile_flops_conv3(const oai_unet* h, int td, int th, int tw, const int overlap_zyx[3], int trimmed);

/* ------------------------------------------------------------------------------------------
 * ICON registration network.  Replaces icon_registration.pretrained_models.
 * OAI_knees_gradICON_model (registration.py:20) + the network part of register_pair (:25).
 * ---------------------------------------------------------------------------------------- */

typedef struct oai_icon oai_icon;

/* One tallUNet2 = UNet2(5, [[2,16,32,64,256,512],[16,32,64,128,256]], 3) in the package's layouts
 * (host, fp32): downConvs[d].weight [Co][Ci][3][3][3], upConvs[d].weight [Ci][Co][4][4][4],
 * batchNorms[d].{weight,bias,running_mean,running_var}, lastConv.weight [3][18][3][3][3]. */
typedef struct oai_icon_unet_params {
    const float* down_w[5]; const float* down_b[5];
    const float* up_w[5];   const float* up_b[5];
    const float* bn_gamma[5]; const float* bn_beta[5]; const float* bn_mean[5]; const float* bn_var[5];
    const float* last_w; const float* last_b;
} oai_icon_unet_params;

/* The registration network is a TREE of the package's wrapper modules around n_nets tallUNet2s -- whatever the checkpoint behind
 * OAI_knees_gradICON_model (registration.py:20) holds; the nesting of `netPhi` / `netPsi` / `net` in its state_dict keys IS this
 * tree (oai_analysis_2_amd/registration.py:parse_icon_tree):
 *   OAI_ICON_FFVF   network_wrappers.FunctionFromVectorField(net = tallUNet2 number a): d = net(A, B) on A's grid;
 *                   transform(x) = x + d when x is the tagged identity map of d's own shape (the isIdentity shortcut), else
 *                   x + sample(d, x)
 *   OAI_ICON_DOWN   DownsampleRegistration(net = node a): the child sees avg_pool3d(A, 2, ceil_mode=True), avg_pool3d(B, ...);
 *                   its transform works in the same [0,1] coordinates
 *   OAI_ICON_TWO    TwoStepRegistration(netPhi = node a, netPsi = node b): phi = netPhi(A, B);
 *                   psi = netPsi(A warped by phi(identity map of A's grid), B); transform(x) = phi(psi(x))
 * nodes[root] is regis_net.  Every node is used exactly once; a child's index differs from its parent's.  A net index may not
 * repeat.  Limits: n_nets, chain length <= OAI_WARP_CHAIN_MAX_FIELDS; every grid a U-Net runs on needs each axis >= 17.
 * Examples (u_k = FFVF(net k)):  SURVEY Appendix A's three-step  TWO(DOWN(TWO(u0,u1)), u2);  "the definition of our final 4 step
 * registration network"  TWO(TWO(DOWN(TWO(u0,u1)), u2), u3);  the gradICON multi-resolution form  TWO(DOWN(TWO(DOWN(u0), u1)), u2). */
enum { OAI_ICON_FFVF = 0, OAI_ICON_DOWN = 1, OAI_ICON_TWO = 2 };
typedef struct oai_icon_node { int kind; int a; int b; } oai_icon_node;

/* BatchNorm3d behind every up-conv (networks.UNet2.batchNorms of the package the reference calls at registration.py:20): pass all four
 * bn_* arrays of a level, or NULL for all four = no normalisation at that level.  icon_registration 1.1.2 is not vendored in the
 * reference tree and one recollection of it has the batchNorms[depth] call commented out in UNet2.forward (the parameters are in the
 * state_dict either way): the caller decides, nothing is assumed silently. */
int oai_icon_create(const oai_icon_unet_params* nets_host, int n_nets, const oai_icon_node* nodes_host, int n_nodes, int root,
                    int D, int H, int W, oai_icon** out);
/* What the tree flattens to: n_nets, the number of launched U-Net passes per direction at each halving level (levels_host[k] =
 * U-Nets on the grid halved k times, k < 8), and the length of the final compose chain. */
int oai_icon_describe(const oai_icon* h, int* n_nets, int* levels_host, int* chain_len);
void oai_icon_destroy(oai_icon* h);
size_t oai_icon_workspace_bytes(const oai_icon* h);

/* phi_AB(identity)[3][D][H][W] for network-resolution images A, B [D][H][W] (one direction of
 * GradientICON.forward followed by model.phi_AB(model.identity_map)). */
int oai_icon_forward(oai_icon* h, const float* A_dev, const float* B_dev, float* phi_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* oai_icon_forward replays its dependent launches (~70 for three U-Nets) as ONE hipGraph (captured on the first call per workspace, on an internal
 * stream; inputs and result have fixed homes inside the workspace, copied in / out around the replay).  oai_icon_set_graph(h, 0)
 * runs the same launches directly.  oai_icon_graph_info: *captured = 1 graph in use, 0 not captured yet, -1 capture failed on this
 * runtime (direct launches are used: same kernels, same results); counts of replays / direct runs. */
int oai_icon_set_graph(oai_icon* h, int enable);
/* Restatement switches of the un-vendored package (defaults = SURVEY Appendix A):
 *   "pad_front" 0|1 (1)  networks.pad_or_crop zero-pads the residual's missing channels in front (1) or behind (0) of the existing ones
 *                        (down path: avg_pool3d(x) has fewer channels than the conv's output). */
int oai_icon_set_option(oai_icon* h, const char* name, int value);
int oai_icon_graph_info(const oai_icon* h, int* captured, long long* replays, long long* direct_runs);

/* One tallUNet2 forward on its own (unit-test seam): out[3][D][H][W] = net number `which` (a, b). */
int oai_icon_unet_forward(oai_icon* h, int which, const float* a_dev, const float* b_dev, int D, int H, int W,
                          float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Iso-surface, smoothing, thickness distance: the step just after the hot path,
 * oai_analysis/mesh_processing.py:298-340, 381-395.
 *   get_mesh():      skimage.measure.marching_cubes(img, level=0.5, spacing, step_size=1)   -> oai_mc_count + oai_mc_emit
 *                    vtkSmoothPolyDataFilter(num_iterations)                                -> oai_mesh_smooth
 *   get_distance():  vtkDistancePolyDataFilter(SignedDistanceOff, second distance on)       -> oai_mesh_point_distance (x2)
 * Conventions (oracle/mesh.py): volume [z][y][x]; inside = value > iso; one vertex per sign-changing grid edge, linear
 * interpolation, (x, y, z) * spacing, ordered by owning voxel then axis; triangles wind outward (inside -> outside), ordered by
 * cell then case-table order; the case table is face-consistent (watertight surface).
 * ---------------------------------------------------------------------------------------- */
/* The 256 x 16 case table (edge ids, -1 terminated) the kernels use, for cross-checks against the oracle's generator. */
int oai_mc_table(signed char* out_256x16_host);
size_t oai_mc_workspace_bytes(int D, int H, int W);
/* Pass 1: classify + prefix sums into the workspace; returns the vertex and triangle counts (synchronises the stream). */
int oai_mc_count(const float* vol_dev, int D, int H, int W, float iso, void* workspace_dev, size_t workspace_bytes,
                 long long* n_verts_host, long long* n_tris_host, void* stream);
/* Pass 2 (same volume, iso and workspace): verts float32 [n_verts][3], faces int32 [n_tris][3]. */
int oai_mc_emit(const float* vol_dev, int D, int H, int W, float iso, const float spacing_xyz_host[3], const void* workspace_dev,
                float* verts_dev, int* faces_dev, void* stream);
/* x <- x + relaxation * (mean of edge neighbours - x), `iterations` Jacobi sweeps over the CSR edge graph
 * (offsets [n_verts+1], neighbours); tmp and out are [n_verts][3] and distinct from the input. */
int oai_mesh_smooth(const float* verts_in_dev, long long n_verts, const int* offsets_dev, const int* neighbours_dev,
                    int iterations, float relaxation, float* tmp_dev, float* verts_out_dev, void* stream);
/* dist[i] = unsigned distance from points[i] to the closest point of the triangle mesh (verts, faces). */
int oai_mesh_point_distance(const float* points_dev, long long n_points, const float* verts_dev, const int* faces_dev,
                            long long n_tris, float* dist_dev, void* stream);
/* Same result with a uniform-grid broad phase (cells of `cell_size` from `grid_lo`, `grid_dims` cells per axis, covering the mesh;
 * cell_size must be >= the longest triangle edge so that a triangle touches at most 8 cells).  Synchronises once. */
size_t oai_mesh_grid_workspace_bytes(const int grid_dims_xyz[3], long long n_tris);
int oai_mesh_point_distance_grid(const float* points_dev, long long n_points, const float* verts_dev, const int* faces_dev,
                                 long long n_tris, const float grid_lo_xyz_host[3], float cell_size, const int grid_dims_xyz_host[3],
                                 void* workspace_dev, size_t workspace_bytes, float* dist_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Atlas thickness map: the step after get_thickness_mesh (SURVEY row L1'), oai_analysis/mesh_processing.py:400-534 as
 * notebooks/FullDemo.ipynb calls it: map_attributes(distance_inner, atlas_inner_mesh), then project_thickness(mapped, mesh_type).
 * Points are float32 [n][3] (x, y, z); sums are fp64 in a fixed order (block partials + one final block, no float atomics), so
 * every result is the same bits from run to run.
 * ---------------------------------------------------------------------------------------- */
/* map_attributes (:400-408): vtkPointInterpolator with VTK 9 defaults (vtkLinearKernel, RADIUS footprint, NormalizeWeights on)
 * and SetNullPointsStrategyToClosestPoint.  out[c][t] = float32(fp64 mean of vals[c][s] over the source points s with
 * |p_s - q_t|^2 <= radius^2), or vals[c][s*] of the closest source point s* (ties: the smallest index) if there is none.
 * vals [n_comp][n_src], out [n_comp][n_tgt].  Brute force over every source point (the cross-check). */
int oai_map_attributes(const float* src_pts_dev, long long n_src, const float* src_vals_dev, int n_comp, const float* tgt_pts_dev,
                       long long n_tgt, double radius, float* out_vals_dev, void* stream);
/* Same result with the source points binned into a uniform grid (cells of `cell_size` >= radius from `grid_lo`, `grid_dims`
 * cells per axis; points outside fall into the border cells), each cell's list ordered by point index; a target point sums the
 * 27 cells around its own, and searches shells of cells for the closest point when that finds nothing.  Mesh_processing.py:400-408. */
size_t oai_point_grid_workspace_bytes(const int grid_dims_xyz[3], long long n_src);
int oai_map_attributes_grid(const float* src_pts_dev, long long n_src, const float* src_vals_dev, int n_comp, const float* tgt_pts_dev,
                            long long n_tgt, double radius, const double grid_lo_xyz_host[3], double cell_size, const int grid_dims_xyz_host[3],
                            void* workspace_dev, size_t workspace_bytes, float* out_vals_dev, void* stream);
/* The footprint that decides mean versus fallback in oai_map_attributes(_grid), for the same arguments minus the values: per target t
 *   count[t]       int32    the source points s with d2 = |p_s - q_t|^2 <= radius^2 (d2: fp64 dx*dx + dy*dy + dz*dz of the widened float32
 *                           coordinates, without contraction: the expression map_attributes tests)
 *   nearest_d2[t]  float64  the minimum d2 over all source points;  nearest_j[t] int32: the smallest index at that minimum
 * map_attributes took the mean exactly where count > 0, and vals[c][nearest_j] where count == 0.  With no source point at a finite
 * distance (NaN or infinite coordinates) nearest_j = -1 and nearest_d2 = +inf.  Integers, compares and a minimum: the grid form and
 * the brute force agree to the bit.  The grid form visits what oai_map_attributes_grid visits (the 27 cells, then shells of cells while
 * count == 0) and takes the same workspace; with count > 0 the nearest point lies inside the 27 cells.  n_src == 0 is an argument
 * error.  Neither call synchronises. */
int oai_point_footprint(const float* src_pts_dev, long long n_src, const float* tgt_pts_dev, long long n_tgt, double radius, int* count_dev,
                        double* nearest_d2_dev, int* nearest_j_dev, void* stream);
int oai_point_footprint_grid(const float* src_pts_dev, long long n_src, const float* tgt_pts_dev, long long n_tgt, double radius,
                             const double grid_lo_xyz_host[3], double cell_size, const int grid_dims_xyz_host[3], void* workspace_dev,
                             size_t workspace_bytes, int* count_dev, double* nearest_d2_dev, int* nearest_j_dev, void* stream);
/* Workspace of the three calls below for n points (mesh_processing.py:411-534). */
size_t oai_thickness_map_workspace_bytes(long long n_points);
/* compute_least_square_circle (:411-447) on (x, y) = (p[col_x], p[col_y]): the centre minimising sum (R_i - mean R)^2, by
 * Gauss-Newton with step halving from the centroid (the reference: scipy leastsq with the centred Jacobian); stops when the step
 * is <= 1e-12 x the rms distance from the centroid, or after 100 steps.  radius = mean R_i.  Synchronises the stream. */
int oai_fit_circle(const float* pts_dev, long long n, int col_x, int col_y, void* workspace_dev, size_t workspace_bytes, double centre_host[2],
                   double* radius_host, int* iterations_host, void* stream);
/* get_projection_from_circle_and_vertice (:459-478), embedded part: angle[i] = atan2(y - c_y, x - c_x), z[i] = p[i][2], fp64. */
int oai_project_circle(const float* pts_dev, long long n, int col_x, int col_y, const double centre_host[2], double* angle_dev, double* z_dev,
                       void* stream);
/* project_thickness, mesh_type "TC" (:486-534): plateaus split at z < 50; per plateau the centred scores on the top-2 axes of its
 * 3x3 scatter matrix (= KernelPCA(n_components=2), linear kernel), each axis signed as sklearn's svd_flip(u) does; the left
 * plateau rotated by -50 degrees, the right one by -160 degrees, its x negated and 50 added to its y.  x, y, thickness_out
 * [n_right + n_left]: the right plateau's points first, each plateau in point order.  An empty plateau is an error.
 * Synchronises the stream. */
int oai_project_plateaus(const float* pts_dev, const float* thickness_dev, long long n, void* workspace_dev, size_t workspace_bytes,
                         double* x_dev, double* y_dev, double* thickness_out_dev, long long* n_right_host, long long* n_left_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Thickness image (csrc/thickness_image.hip): map_attributes puts every knee's thickness on the atlas inner mesh, so all knees share
 * the atlas' 2-D projection; it is rasterised once per atlas and each knee's image is one gather.  uv is float64 [n_pts][2] in mesh
 * point order.  Pixel (j, i) of the [height][width] image has its centre at (lo[0] + (i + 0.5) step[0], lo[1] + (j + 0.5) step[1]); one
 * step per axis (the axes need not share a unit).  All decisions in fp64 without contraction, restated in tests/thickness_image_ref.py.
 * ---------------------------------------------------------------------------------------- */
/* Workspace of oai_thickness_image_build (one box per face); 0 for no faces or an empty image. */
size_t oai_thickness_image_workspace_bytes(long long n_faces, int height, int width);
/* Face f = (a, b, c) with area = (B.u-A.u)(C.v-A.v) - (B.v-A.v)(C.u-A.u) is skipped if face_skip[f] (NULL: none), if an index lies
 * outside [0, n_pts), if a coordinate is not finite or if area == 0.  Edge functions at the centre P:
 * e0 = (C.u-B.u)(P.v-B.v) - (C.v-B.v)(P.u-B.u), e1 likewise on C->A, e2 on A->B, all negated when area < 0; f covers the pixel iff
 * e0 >= 0 && e1 >= 0 && e2 >= 0 (edges inclusive).  owner = the SMALLEST covering face index (integer atomicMin: the same bits on every
 * run) or -1; for the owner, corners = (a, b, c) and weights = e_k / ((e0 + e1) + e2); corners and weights are 0 where owner is -1.
 * n_covered_host = the number of pixels with an owner.  Synchronises the stream. */
int oai_thickness_image_build(const double* uv_dev, long long n_pts, const int* faces_dev, long long n_faces, const unsigned char* face_skip_dev,
                              const double lo_host[2], const double step_host[2], int height, int width, void* workspace_dev,
                              size_t workspace_bytes, int* owner_dev, int* corners_dev, double* weights_dev, long long* n_covered_host,
                              void* stream);
/* image[k][j][i] = (float)((w0 t[a] + w1 t[b]) + w2 t[c]) with t = values[k] widened to double, NaN (0x7fc00000) where owner < 0;
 * values [n_knees][n_pts], image [n_knees][height][width].  A pure gather: one thread per pixel and knee. */
int oai_thickness_image_apply(const int* owner_dev, const int* corners_dev, const double* weights_dev, int height, int width,
                              const float* values_dev, long long n_pts, int n_knees, float* image_dev, void* stream);

/* ---- inner / outer split of a cartilage surface (mesh_processing.py:197-294, 353-378; csrc/mesh_split.hip) ----
 * KMeans(n_clusters=2, algorithm="lloyd") of scikit-learn >= 1.4 restated in fp64: FC = three x slabs of 9 features, n_init 5 each;
 * TC = one fit of 6 features, n_init 1.  The host draws each fit's random numbers (numpy RandomState(5): choice, then uniform(size=2),
 * per init) from the slab sizes that oai_mesh_split_features returns; no RNG runs on the device. */
#define OAI_MESH_FC 0
#define OAI_MESH_TC 1
/* Workspace of oai_mesh_split_features + oai_mesh_split_kmeans with n_init runs per slab (one buffer, kept between the two calls):
 * the slabs' features (n_faces rows, FC: + n_faces / 64 + 64 for faces on a slab seam) and n_init label / distance rows.  0 for bad
 * arguments. */
size_t oai_mesh_split_workspace_bytes(long long n_verts, long long n_faces, int mesh_type, int n_init);
/* Per face: centroid (a + b + c) / 3 and unit normal cross(b - a, c - a) / |.| (0 for a degenerate face) as fp64 [n_faces][3],
 * bit-identical to get_cell_centroid / get_cell_normals; then cn = (c - mean c) / (max c - min c), the features and the slabs
 * (FC: lower <= cn_x < lower + step, a face in no slab keeps side 0).  slab_counts_host[s] = faces of slab s (TC: [n_faces, 0, 0]).
 * Synchronises the stream once. */
int oai_mesh_split_features(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, int mesh_type,
                            void* workspace_dev, size_t workspace_bytes, double* centroids_dev, double* normals_dev,
                            long long slab_counts_host[3], void* stream);
/* The fits, after oai_mesh_split_features on the same workspace: one workgroup per (slab, init) run (k-means++ with 2 local trials,
 * Lloyd to labels unchanged or sum |shift|^2 <= 1e-4 mean var, at most max_iter), fit()'s best-of-init rule, the orientation.
 * first_centre_host[s * n_init + i] / uniforms_host[2 (s * n_init + i) + t]: run i of slab s.  side_dev: int8 [n_faces] in {-1, 0, +1}
 * (-1 inner).  n_iter_host[s]: the chosen run's iteration count.  A slab with < 2 faces is an argument error; a cluster that empties
 * during the iterations (sklearn relocates a point) is an error.  Synchronises the stream once. */
int oai_mesh_split_kmeans(long long n_faces, int mesh_type, void* workspace_dev, size_t workspace_bytes, const double* normals_dev, int n_init,
                          int max_iter, const long long slab_counts_host[3], const long long* first_centre_host, const double* uniforms_host,
                          signed char* side_dev, int* n_iter_host, void* stream);
/* get_vtk_sub_mesh (:150-194) of the faces with side_dev[i] == which: faces in ascending index order (face_idx_out), vertices in order of
 * first use in the flattened face list, indices remapped.  Outputs sized for the worst case ([n_verts][3], [n_faces][3], [n_faces]);
 * the counts come back to the host.  Synchronises the stream twice. */
size_t oai_mesh_submesh_workspace_bytes(long long n_verts, long long n_faces);
int oai_mesh_submesh(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, const signed char* side_dev, int which,
                     void* workspace_dev, size_t workspace_bytes, float* verts_out_dev, int* faces_out_dev, int* face_idx_out_dev,
                     long long* n_verts_out_host, long long* n_faces_out_host, void* stream);

/* ---- mesh graph steps of get_mesh / point_distance (mesh_processing.py:108-141; csrc/mesh_graph.hip) ----
 * The host graph code between the mesh kernels, on the device: with these a caller goes from a probability map to a thickness mesh
 * without a host round trip.  Faces are int32 [n_faces][3]; every face index must lie in [0, n_verts) (an index
 * outside is an argument error, found before anything is written from it).  Results are exact, the same bits on every run. */
/* Connected components of the face graph (two vertices are joined when they share a face): label_dev[v] = the smallest vertex index
 * of v's component; an unreferenced vertex is its own component.  Hook / jump rounds, one launch each; the "changed" flags are read
 * every 4 rounds (synchronises the stream once per 4 rounds).  rounds_host (may be null): hook / jump rounds up to and including the
 * first that changed nothing (0 for n_faces = 0). */
size_t oai_mesh_components_workspace_bytes(long long n_verts, long long n_faces);
int oai_mesh_components(const int* faces_dev, long long n_faces, long long n_verts, void* workspace_dev, size_t workspace_bytes, int* label_dev,
                        int* rounds_host, void* stream);
/* keep_large_regions (get_vtk_mesh's connectivity loop, :114-141): the faces of components with more than min_cells faces (a face
 * counts for the component of its first vertex), in their original order; the vertices they use in ascending original index,
 * remapped.  Outputs sized for the worst case ([n_verts][3], [n_faces][3]); the counts come back to the host.  Synchronises the
 * stream (as oai_mesh_components, then once). */
size_t oai_mesh_keep_large_regions_workspace_bytes(long long n_verts, long long n_faces);
int oai_mesh_keep_large_regions(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, long long min_cells,
                                void* workspace_dev, size_t workspace_bytes, float* verts_out_dev, int* faces_out_dev, long long* n_verts_out_host,
                                long long* n_faces_out_host, void* stream);
/* vertex_adjacency (:108): the CSR edge graph of oai_mesh_smooth, offsets [n_verts + 1] and neighbours (capacity 6 n_faces), each
 * vertex's neighbours ascending and unique; the self-loop of a degenerate face [a, a, b] is kept, an isolated vertex has degree 0.
 * n_nbrs_host = offsets[n_verts].  Synchronises the stream once. */
size_t oai_mesh_adjacency_workspace_bytes(long long n_verts, long long n_faces);
int oai_mesh_adjacency(const int* faces_dev, long long n_faces, long long n_verts, void* workspace_dev, size_t workspace_bytes, int* offsets_dev,
                       int* nbrs_dev, long long* n_nbrs_host, void* stream);
/* What oai_mesh_point_distance_grid's caller derives from the mesh (point_distance): out7_dev (fp64, device) = the float32 bounding
 * box lo xyz, hi xyz (min / max over every vertex), then the largest squared edge length over the faces' three edges in fp64,
 * (dx*dx + dy*dy) + dz*dz with no contraction (numpy's norm before its sqrt; 0 for no faces, NaN if a face indexes outside the
 * vertices).  Does not synchronise. */
size_t oai_mesh_grid_params_workspace_bytes(void);
int oai_mesh_grid_params(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, void* workspace_dev,
                         size_t workspace_bytes, double* out7_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Cuberille iso-surface: get_mesh_from_probability_map (oai_analysis/mesh_processing.py:343-350), which calls
 *   itk.cuberille_image_to_mesh_filter(image, generate_triangle_faces=True, iso_surface_value=0.5,
 *       project_vertices_to_iso_surface=True, project_vertex_surface_distance_threshold=0.05)
 * Restated, unpinned (ITK absent; DESIGN.md 1 lists the recalled points).  csrc/cuberille.hip, tests/cuberille_ref.py.
 *   - volume [z][y][x] fp32; a voxel is inside when value >= iso; a neighbour off the grid is outside (closed surfaces).
 *   - one quad per (inside voxel, outside face neighbour): voxels in raster order (x fastest), then neighbours -z -y -x +x +y +z.
 *   - one vertex per lattice point a face uses; lattice point (i, j, k), i in [0, W] etc., lies at continuous index
 *     (i - 1/2, j - 1/2, k - 1/2).  Vertices are numbered in order of first use (faces in order, corners in order) and are not
 *     split where voxels touch at an edge or corner only: such contacts give non-manifold edges / vertices.
 *   - a face on axis a with in-plane axes (b, c) = x:(y,z) y:(z,x) z:(x,y) has corners (b, c) = (0,0) (1,0) (1,1) (0,1) on the +a
 *     side and (0,0) (0,1) (1,1) (1,0) on the -a side (normals point from inside to outside in index space).  Quad f = (q0 q1 q2 q3)
 *     gives triangles 2f = (q0 q1 q2) and 2f+1 = (q0 q2 q3).  flip_winding (the caller sets it when det(direction) < 0) keeps each
 *     polygon's first vertex and reverses the rest: (q0 q2 q1), (q0 q3 q2); quads (q0 q3 q2 q1).  Vertex numbering is unaffected.
 *   - coordinates: u = spacing * c_xyz, p = origin + direction @ u, in fp64, stored fp32.
 *   - projection (per vertex, fp64, no contraction): c = M (p - origin) with M = inv(direction diag(spacing)) as given; value =
 *     trilinear interpolation at c clamped to [0, n-1] per axis; gradient = per-voxel central differences with replicated borders,
 *     (f[i+1] - f[i-1]) / (2 s_axis), interpolated at the same c, then direction @ it.  With step = L, k = 0:
 *       loop: g = grad(p); if |g| == 0 stop; m = value(p) - iso; done = |m| <= threshold;
 *             if done and not move_after_converged stop; p += (m < 0 ? step : -step) * (g / |g|);
 *             k += 1; done |= k > max_steps; step *= relaxation; if done stop
 *     L = step_length, or 0.25 * max(spacing) when step_length < 0.  steps_dev[v] = k.
 * geometry_host[24] = origin xyz, spacing xyz, direction (row-major 3x3), M (row-major 3x3).
 * ---------------------------------------------------------------------------------------- */
/* 0 when an axis is < 1 voxel or the volume is too large for 32-bit corner slots. */
size_t oai_cuberille_workspace_bytes(int D, int H, int W);
/* Classify, first use of every lattice point, vertex numbering; returns the vertex and quad counts (synchronises the stream). */
int oai_cuberille_count(const float* vol_dev, int D, int H, int W, float iso, void* workspace_dev, size_t workspace_bytes,
                        long long* n_verts_host, long long* n_faces_host, void* stream);
/* After oai_cuberille_count on the same volume, iso and workspace, with the counts it returned: verts float32 [n_verts][3], faces int32
 * [2 n_faces][3] (triangles != 0) or [n_faces][4]; steps_dev (may be null) int32 [n_verts].  threshold, step_length, relaxation and
 * max_steps are checked and used only when project != 0.  Does not synchronise. */
int oai_cuberille_emit(const float* vol_dev, int D, int H, int W, float iso, const double geometry_host[24], int flip_winding, int triangles,
                       int project, double threshold, double step_length, double relaxation, int max_steps, int move_after_converged,
                       void* workspace_dev, size_t workspace_bytes, long long n_verts, long long n_faces, float* verts_dev, int* faces_dev,
                       int* steps_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Points pushed through phi: the point form of oai_resample_maps_through_phi (csrc/mesh_transform.hip, tests/mesh_transform_ref.py).
 * phi maps atlas (B) points to patient (A) points, so the vertices of a mesh extracted on the atlas grid land on the patient's own
 * surface.  The reference would do this step with itk.transform_mesh_filter and the registration's CompositeTransform, if at all;
 * restated from ITK's documented composite-transform behaviour and unpinned (ITK absent), like the resample (oracle/resample.py).
 * Per point p (float32 xyz), every coordinate in fp64 without contraction:
 *   x = point_to_net(p);  inside = x in [-0.5, n - 0.5) on all three axes (the half-open test of the resample; false for a NaN);
 *   d = the displacement at the 8 corners clamped to the buffer -- rebuilt from phi by itk_disp of csrc/phi_field.h, the function
 *       behind every rebuild in the library (fp32 (phi - identity_coord) * (n - 1), widened),
 *       xyz components: at a lattice point the value oai_phi_to_itk_displacement stores -- lerped along x, then y, then z;
 *   x2 = x + (inside ? d : 0)   (identity outside the field's buffer: ITK's DisplacementFieldTransform);  out = float32(net_to_out(x2)).
 * phi_dev fp32 [3][Dn][Hn][Wn] in [0,1] units, channels z, y, x; out_dev float32 [n][3]; inside_dev (may be null) one byte per point,
 * 1 = inside.  n = 0 is a successful no-op; an axis of phi below 2 voxels is an argument error.  out_dev may not alias pts_dev.  Does
 * not synchronise.
 * ---------------------------------------------------------------------------------------- */
int oai_transform_points_through_phi(const float* pts_dev, long long n, const float* phi_dev, int Dn, int Hn, int Wn,
                                     const oai_affine* point_to_net, const oai_affine* net_to_out, float* out_dev, unsigned char* inside_dev,
                                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Registration QC (csrc/phi_jacobian.hip, tests/phi_jacobian_ref.py): the Jacobian determinant of phi, its fold count, and the overlap
 * counts of two thresholded maps.  The fold definition is that of icon_registration.losses.flips (backward differences, negative
 * determinant), restated as recalled and unpinned: icon_registration is absent.
 *
 * oai_phi_jacobian: phi_dev fp32 [3][D][H][W] in [0,1] units, channels z, y, x (ITK component c = channel 2 - c), identity =
 * float32((double)i * 1/(n-1)).  One determinant per cell (z,y,x), z in [1,D), y in [1,H), x in [1,W), on the displacement in network
 * voxels, contraction off:
 *   u_c(p)  = (double)((phi[2-c][p] - identity_c(p)) * (float)(n_c - 1))          itk_disp of csrc/phi_field.h, as oai_phi_to_itk_displacement
 *   J[r][k] = delta_rk + (u_r(p) - u_r(p - e_k))                                  fp64; r, k over (x, y, z)
 *   det     = (J00*(J11*J22 - J12*J21) - J01*(J10*J22 - J12*J20)) + J02*(J10*J21 - J11*J20)
 * (the displacement form reads exactly 1 on the identity map; raw phi differences do not, float32 coordinates not being equidistant).
 * det_out_dev (may be null): float32 [D-1][H-1][W-1], the rounded determinant.  stats_dev: double[7] on the device --
 *   [0] cells = (D-1)(H-1)(W-1)   [1] folds: det < 0 on the fp64 value   [2] cells with a non-finite determinant, left out of all the others
 *   [3] min  [4] max  (+inf / -inf when no cell is finite)   [5] sum of det   [6] sum of det^2
 * Reduced in the fixed order of csrc/ordered_reduce.h (per-block partials in the workspace, a second kernel over them): no atomics, a
 * block count that depends on the shape only, so the stats are bit-reproducible and do not depend on det_out_dev.  Does not synchronise.  Every axis must be >= 2.
 * ---------------------------------------------------------------------------------------- */
/* 0 when an axis is below 2 voxels. */
size_t oai_phi_jacobian_workspace_bytes(int D, int H, int W);
int oai_phi_jacobian(const float* phi_dev, int D, int H, int W, float* det_out_dev, void* workspace_dev, size_t workspace_bytes,
                     double* stats_dev, void* stream);
/* oai_mask_overlap: a_dev, b_dev float32 [n] (b_dev may be null: the set B is empty).  A value belongs to its set when it is finite and
 * > threshold (the segmentation's rule); a non-finite value is in no set.  counts_dev: long long[4] on the device -- |A|, |B|, |A and B|,
 * positions where a or b is non-finite.  Integer arithmetic: exact.  n = 0 gives zeros (and needs no workspace).  Does not synchronise. */
size_t oai_mask_overlap_workspace_bytes(long long n);
int oai_mask_overlap(const float* a_dev, const float* b_dev, long long n, float threshold, void* workspace_dev, size_t workspace_bytes,
                     long long* counts_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * The inverse of phi (csrc/phi_inverse.hip, tests/phi_inverse_ref.py): patient (A) points taken to the atlas (B), the direction phi
 * does not provide.  A numerical inverse of the map that is held, exact up to a stated residual: what itk.Transform.GetInverseTransform
 * means for a displacement field, restated from ITK's documented behaviour and unpinned (ITK absent); not the network's phi_BA.
 * The forward map in network index space is that of oai_transform_points_through_phi,
 *   T(x) = x + (inside(x) ? u(x) : 0),   u = itk_disp at the 8 clamped corners lerped along x, then y, then z,
 * and one device solver finds x with T(x) = y, in fp64 without contraction:
 *   x = y;  at most max_iter times:
 *     d, G = u(x), grad u(x) when inside(x), else zero; G is the exact gradient of the trilinear interpolant from the same 8 corners
 *            (the column of an axis that clamp_split clamped is zero);
 *     r = (x + d) - y;  converged when max_c |r_c| <= tol;
 *     J = I + G;  det as in oai_phi_jacobian;  s = J^-1 r by the adjugate when |det| > 1e-3, else s = r (a fixed-point step);
 *     stop as unconverged when a component of s is not finite, else x -= s.
 * Status per point: 1 = converged with x inside the buffer; 2 = converged at an x outside it, where T is the identity; 0 = not
 * converged within max_iter, and the result is then x = y: the point is moved by the affines alone, the forward transform's convention
 * for "outside".  Newton, because the plain fixed point diverges wherever phi stretches by a factor of 2 or more.  tol is in network
 * voxels (1e-7 is two orders below the float32 quantum of a stored map, 2^-24 (n - 1)); max_iter >= 1 and tol > 0 are checked.
 *
 * oai_inverse_points_through_phi: out = float32(net_to_out(solve(point_to_net(p)))) per point p (float32 xyz); out_dev float32 [n][3];
 * status_dev (may be null) one byte per point.  n = 0 is a successful no-op; an axis of phi below 2 voxels is an argument error.
 * out_dev may not alias pts_dev.  Does not synchronise.
 *
 * oai_invert_phi: the dense inverse on phi's own lattice.  For every lattice point y, psi[2-c][y] = float32(x_c * (1/(n_c - 1))), phi's
 * storage convention: psi is a phi, and oai_resample_maps_through_phi, oai_transform_points_through_phi and oai_phi_jacobian read it
 * unchanged.  An unconverged point holds its identity coordinate.  psi_out_dev fp32 [3][D][H][W] (may not alias phi_dev);
 * status_out_dev (may be null) [D][H][W] bytes.  stats_dev: double[6] on the device --
 *   [0] points = D H W   [1] unconverged   [2] converged outside the buffer   [3] max |r| over the converged points
 *   [4] sum over all points of the evaluations of T   [5] their maximum
 * Reduced in the fixed order of csrc/ordered_reduce.h (per-block partials in the workspace, a second kernel over them): no atomics, a
 * block count that depends on the shape only, so the stats are bit-reproducible and do not depend on status_out_dev.  Does not synchronise.
 * ---------------------------------------------------------------------------------------- */
int oai_inverse_points_through_phi(const float* pts_dev, long long n, const float* phi_dev, int Dn, int Hn, int Wn,
                                   const oai_affine* point_to_net, const oai_affine* net_to_out, int max_iter, double tol, float* out_dev,
                                   unsigned char* status_dev, void* stream);
/* 0 when an axis is below 2 voxels. */
size_t oai_invert_phi_workspace_bytes(int D, int H, int W);
int oai_invert_phi(const float* phi_dev, int D, int H, int W, int max_iter, double tol, float* psi_out_dev, unsigned char* status_out_dev,
                   void* workspace_dev, size_t workspace_bytes, double* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Surface-distance QC (csrc/edt.hip, tests/edt_ref.py): the exact Euclidean distance transform of a binary volume with anisotropic
 * spacing, the surface of a thresholded map, and the surface-distance figures of two surfaces (ASSD, Hausdorff, HD95).  The
 * definitions -- the surface rule and the pooled percentile -- are MedPy's (medpy.metric.binary: __surface_distances, assd, hd, hd95)
 * on scipy.ndimage, restated and checked against scipy on the CPU (tests/test_edt_cpu.py); they are not tied to ITK's
 * SignedMaurerDistanceMapImageFilter, ITK being absent.  All volumes are [z][y][x]; spacing_xyz is (x, y, z).
 *
 * oai_mask_surface: map_dev float32 [D][H][W], out_dev one byte per voxel.  A voxel is in the set when its value is finite and
 * > threshold (oai_mask_overlap's rule).  mode 0: out = 1 for every voxel of the set, else 0.  mode 1: the surface -- a voxel of the set
 * with at least one of its six face neighbours not in the set or outside the volume, which is A ^ binary_erosion(A, 6-connectivity,
 * border_value=0).  mode 2: the complement of mode 0.  Every axis in [1, 32767].  Does not synchronise.
 *
 * oai_edt: feature_dev one byte per voxel, a feature where != 0.  For every voxel p the squared distance is the minimum over all
 * feature voxels q of the canonical expression, in fp64 without contraction:
 *   tx = (double)(px - qx) * sx;  ty = (double)(py - qy) * sy;  tz = (double)(pz - qz) * sz;      sq = (tx*tx + ty*ty) + tz*tz
 * to the bit (what scipy.ndimage.distance_transform_edt(~features, sampling=(sz, sy, sx)) squares to within 1e-15 relative); +inf
 * everywhere when there is no feature.  Computed separably with exhaustive line scans and an exact cut-off -- IEEE rounding is monotone,
 * a <= b  =>  fl(a + c) <= fl(b + c), so the per-line minimum of the partial sum carries the minimum of the whole -- never by parabola
 * intersections in floating point.
 *   sq_out_dev[p] (may be null) = sq
 *   dist_dev[p] = (accumulate ? dist_dev[p] : 0.0f) + scale * (float)sqrt(sq)          float32 operations, no contraction
 *   n_features_dev (may be null): the number of feature voxels, on the device
 * scale is 1 or -1: a second call on the complement with scale = -1, accumulate = 1 turns the first call's map of the set into the
 * signed map, positive outside the set and negative inside, scipy's edt(~m) - edt(m).  Every axis in [1, 32767], every spacing finite
 * and > 0.  The workspace holds the passes' integer offsets, 6 bytes per voxel and 4 per row.  Does not synchronise.
 *
 * oai_surface_distance: surf_*_dev one byte per voxel (oai_mask_surface, mode 1), dist_to_*_dev float32 (oai_edt of the other
 * surface), n voxels.  The directed distances are d(A->B) = dist_to_b[p] for every p with surf_a[p] != 0, and likewise d(B->A).
 * out_dev: double[8] on the device --
 *   [0] n_A   [1] n_B   [2] sum d(A->B)   [3] sum d(B->A)   [4] max d(A->B)   [5] max d(B->A)   [6], [7] the requested percentiles
 * The sums are fp64 sums of the widened float32 distances in the fixed order of csrc/ordered_reduce.h, which tests/ordered_reduce_ref.py
 * restates and tests/test_edt_gpu.py pins to the bit -- no float atomics and a block count that depends on n only.  The percentiles
 * (percentiles: n_percentiles = 0..2 host floats in [0, 100]) are np.percentile of the pooled array concat(d(A->B), d(B->A)), MedPy's
 * hd95: exact order statistics by the 4-pass radix select of csrc/radix_select.h and numpy's float32 interpolation, as oai_image_normalize,
 * with the ranks computed on the device because n_A + n_B is known there only.  When n_A = 0 or n_B = 0, [2]..[7] are NaN and the
 * counts are still reported; a percentile slot that was not asked for is NaN.  ASSD = ([2] + [3]) / ([0] + [1]), Hausdorff =
 * max([4], [5]).  Does not synchronise.
 * ---------------------------------------------------------------------------------------- */
int oai_mask_surface(const float* map_dev, int D, int H, int W, float threshold, int mode, unsigned char* out_dev, void* stream);
/* 0 when an axis is outside [1, 32767]. */
size_t oai_edt_workspace_bytes(int D, int H, int W);
int oai_edt(const unsigned char* feature_dev, int D, int H, int W, const double spacing_xyz[3], float scale, int accumulate, float* dist_dev,
            double* sq_out_dev, void* workspace_dev, size_t workspace_bytes, long long* n_features_dev, void* stream);
/* 0 when n < 0. */
size_t oai_surface_distance_workspace_bytes(long long n);
int oai_surface_distance(const unsigned char* surf_a_dev, const float* dist_to_b_dev, const unsigned char* surf_b_dev, const float* dist_to_a_dev,
                         long long n, const float* percentiles, int n_percentiles, void* workspace_dev, size_t workspace_bytes, double* out_dev,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Image-similarity QC (csrc/similarity.hip, tests/similarity_ref.py): how alike two float32 images on one grid are -- the moments behind
 * Pearson's r (NCC) and the mean squared error, the joint histogram and its entropies (mutual information), and the local normalised
 * cross-correlation (LNCC) that ICON trains on.  ICON's LNCC form, its sigma and eps are restated as recalled and unpinned:
 * icon_registration is absent.  fp64 without contraction; every floating sum in the fixed order of csrc/ordered_reduce.h (per-block slots
 * in the workspace, a one-block finish kernel, a block count that depends on the shape only): bit-reproducible, and the same with and
 * without the optional outputs.  mask_dev (may be null everywhere): one byte per position, a position takes part when its byte is
 * non-zero.  No entry point synchronises.
 *
 * oai_image_moments: a_dev, b_dev float32 [n].  A position is counted when the mask admits it and both values are finite.
 * stats_dev: double[8] on the device --
 *   [0] counted positions   [1] admitted positions left out for a non-finite value
 *   [2] sum a   [3] sum b   [4] sum a*a   [5] sum b*b   [6] sum a*b   [7] sum (a - b)^2
 * every term formed in fp64 from the float32 values (the three products are exact there).  Thread g of min(2048, ceil(n / 1024)) blocks
 * of 256 adds positions g, g + threads, ... in that order.  n = 0 gives zeros and needs no workspace.
 *
 * oai_joint_histogram: hist_dev long long [bins*bins + 1] on the device, zeroed by the call.  The bin of a value x is
 *   min((int)((clamp(x, lo, hi) - lo) * scale), bins - 1),   scale = (float)(bins / ((double)hi - (double)lo)),
 * every operation in float32: a finite value outside [lo, hi] goes to an end bin (np.histogram2d drops it).  hist[ia*bins + ib] counts
 * the admitted pairs with both values finite; hist[bins*bins] counts the admitted positions skipped for a non-finite value.  Integer
 * counts, exact in any order: a per-block LDS table up to 64 bins, one 64-bit atomic add per non-zero cell when a block retires; above
 * 64 bins, 64-bit global atomics.
 * 1 <= bins <= 128, hi > lo, n <= 2^40.
 *
 * oai_histogram_entropies: hist_dev as above.  out_dev: double[4] on the device -- N = the sum of the bins*bins counts, H_A, H_B, H_AB
 * with H = 0 - sum over the non-zero cells in index order of p * log(p), p = (double)c / (double)N, natural logarithm; the marginals by
 * integer sums.  N = 0 gives N = 0 and three NaNs.  One block.
 *
 * oai_lncc: a_dev, b_dev float32 [D][H][W].  The five channels a, b, a*a, b*b, a*b are formed in fp64 and filtered along x, then y,
 * then z, each pass
 *   acc = 0;  for j = 0 .. 2 radius:  acc = acc + taps[j] * v[reflect(i + j - radius)]            (multiply and add apart, j ascending)
 * with reflect that of np.pad(mode="reflect") / scipy's mode="mirror" (no repeated edge sample) and nothing rounded to float32 between
 * the passes.  Per voxel, with E the filtered channels:
 *   cov = Eab - Ea*Eb;  va = Eaa - Ea*Ea;  vb = Ebb - Eb*Eb;  cc = cov / sqrt((va + eps) * (vb + eps))
 * taps_host: 2 radius + 1 doubles on the HOST (the caller's Gaussian, so that no exp is evaluated in two places).  cc_out_dev (may be
 * null): double [D][H][W], every voxel, masked or not.  stats_dev: double[6] on the device --
 *   [0] counted voxels (admitted, cc finite)   [1] admitted voxels left out for a non-finite cc
 *   [2] sum cc   [3] sum cc^2   [4] min   [5] max  (NaN when no voxel is counted)
 * one voxel per thread, block k = voxels [256 k, 256 k + 256).  0 <= radius <= 32 and every axis > radius.  The workspace holds two
 * sets of five fp64 volumes (80 B per voxel).
 * ---------------------------------------------------------------------------------------- */
/* 0 when n <= 0. */
size_t oai_image_moments_workspace_bytes(long long n);
int oai_image_moments(const float* a_dev, const float* b_dev, long long n, const unsigned char* mask_dev, void* workspace_dev,
                      size_t workspace_bytes, double* stats_dev, void* stream);
int oai_joint_histogram(const float* a_dev, const float* b_dev, long long n, const float range_a[2], const float range_b[2], int bins,
                        const unsigned char* mask_dev, long long* hist_dev, void* stream);
int oai_histogram_entropies(const long long* hist_dev, int bins, double* out_dev, void* stream);
/* 0 when an axis is below 1 voxel. */
size_t oai_lncc_workspace_bytes(int D, int H, int W);
int oai_lncc(const float* a_dev, const float* b_dev, int D, int H, int W, const double* taps_host, int radius, double eps,
             const unsigned char* mask_dev, double* cc_out_dev, void* workspace_dev, size_t workspace_bytes, double* stats_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation-shape QC (csrc/components.hip, tests/components_ref.py): 3-D connected-component labelling of a voxel set, the
 * reference-free check of a segmentation -- how many pieces, how much of it in the largest, how much in islands, how many closed
 * cavities -- and the primitive that cleans a mask.  The numbering is that of scipy.ndimage.label(mask,
 * generate_binary_structure(3, r)), r = 1, 2, 3, checked against scipy on the CPU (tests/test_components_cpu.py).
 *
 * oai_label_components.  The set: exactly one of map_dev and mask_dev is non-null.  map_dev float32 [D][H][W]: a voxel is in the set
 * when its value is finite and > threshold (the rule of oai_mask_overlap and oai_mask_surface; the threshold may not be NaN).
 * mask_dev one byte per voxel: in the set when the byte is != 0.  complement != 0 labels the voxels that are NOT in the set; a
 * non-finite value is then in the complement, as in mode 2 of oai_mask_surface.  connectivity is 6, 18 or 26: two voxels of the
 * labelled set are joined when they share a face; a face or an edge; a face, an edge or a corner.  A component is a class of the
 * transitive closure.
 *   labels_dev (may be null) int32 [D][H][W]: 0 outside the labelled set; the components are numbered 1..K in raster order of each
 *     component's first voxel (its voxel with the smallest index (z H + y) W + x).
 *   size_dev (may be null) int32 [D][H][W]: the voxel count of the component that the voxel belongs to, 0 outside the labelled set --
 *     so that "drop everything below n voxels" and "keep the largest" are element-wise operations on the device.
 *   summary_dev: long long[12] on the device, integers and therefore exact --
 *     [0] voxels = D H W   [1] voxels of the labelled set   [2] K, the number of components
 *     [3] the size of the largest component (0 when K = 0)   [4] its label, on a tie the smallest (0 when K = 0)
 *     [5] the size of the second largest (0 when K < 2; equal to [3] on a tie)
 *     [6] components with size < min_voxels   [7] the voxels in them
 *     [8] components that touch the border of the volume (a voxel with an index 0 or n - 1 on some axis)   [9] the voxels in them
 *     [10] non-finite positions of map_dev (0 with mask_dev)   [11] 0
 *   The summary does not depend on labels_dev or size_dev being null.
 * How: a union-find over the voxels whose representative is the SMALLEST LINEAR INDEX of the component.  A parent link only ever
 * moves to a smaller index of the same component (integer atomicMin), so every tree ends rooted at its component's first voxel
 * whatever order the workgroups ran in: labels, sizes and summary are a function of the input alone, bit-identical from run to run.
 * A brick of 4 x 4 x 64 voxels is merged in LDS; neighbouring bricks are merged across their faces (for 18 and 26 also across their
 * edges and corners) in global memory, one returning atomic per pair of voxels whose roots still differ; parents are flattened, the
 * size and the border flag of each component accumulated at its root's own index in the workspace (integer atomicAdd / atomicOr); the
 * label is 1 + the exclusive scan of the root flags over the volume (per-block counts, one block over the block partials in the
 * order of csrc/ordered_reduce.h, a last pass that writes labels_dev and size_dev).  No floating-point value is reduced.  No
 * rounds: nothing can fail to converge, no flag is read back, and stream order is the only grid-wide synchronisation.  Does not
 * synchronise.  Every axis in [1, 32767] and D H W <= 2^31 - 1 (indices are int32); min_voxels >= 0.  The workspace holds the parents
 * and the per-root accumulators, 8 bytes per voxel, and about 0.1 byte per voxel of block partials.
 *
 * oai_component_sizes: labels_dev int32 [n].  sizes_dev[k - 1] = the number of positions with label k, k = 1..n_components, long long
 * on the device; the call clears the table itself.  A label outside 0..n_components is ignored.  n = 0 or n_components = 0 is a
 * successful no-op.  Integer atomicAdd: exact in any order.  Does not synchronise.
 * ---------------------------------------------------------------------------------------- */
/* 0 when an axis is outside [1, 32767] or D*H*W > 2^31 - 1. */
size_t oai_label_components_workspace_bytes(int D, int H, int W);
int oai_label_components(const float* map_dev, const unsigned char* mask_dev, int D, int H, int W, float threshold, int complement,
                         int connectivity, long long min_voxels, int* labels_dev, int* size_dev, void* workspace_dev, size_t workspace_bytes,
                         long long* summary_dev, void* stream);
int oai_component_sizes(const int* labels_dev, long long n, long long n_components, long long* sizes_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Thickness QC (csrc/local_thickness.hip, tests/local_thickness_ref.py): the local thickness of a voxel set (Hildebrand and
 * Ruegsegger 1997; what BoneJ and porespy implement) -- at a voxel the diameter of the largest ball that contains the voxel and stays
 * inside the object -- and the statistics of a float32 field under a byte mask.  It needs no mesh, no inner/outer split, no atlas and
 * no phi: an independent figure beside the mesh-based thickness.  All volumes are [z][y][x]; spacing_xyz is (x, y, z).
 *
 * oai_local_thickness: rsq_dev float64 [D][H][W], a squared-radius field from any source (the first is oai_edt's sq of the set's
 * complement).  A voxel q is a centre when rsq[q] is finite and > 0; NaN, +-inf, zero and negative entries are not.  For every centre p
 *   tx = (double)(px - qx) * sx;  ty = (double)(py - qy) * sy;  tz = (double)(pz - qz) * sz;      d2 = (tx*tx + ty*ty) + tz*tz
 *   sq_out[p] = max over the centres q with d2 < rsq[q] of rsq[q]
 *   thick[p]  = 2.0f * (float)sqrt(sq_out[p])
 * d2 being oai_edt's canonical expression, in fp64 without contraction.  p covers itself, so sq_out[p] >= rsq[p].  sq_out[p] = 0 and
 * thick[p] = 0 where p is not a centre.  The inequality is strict: with rsq the squared distance to the complement, the ball d < D(q)
 * holds no background voxel, and <= would reach the nearest one.  Only fp64 compares and a max are involved, so the result does not
 * depend on the order of execution and is bit-identical to the brute force over all pairs.
 *   sq_out_dev (may be null) float64, thick_dev float32, both [D][H][W]
 *   stats_dev (may be null): long long[4] on the device --
 *     [0] centres   [1] voxel tests done: the sum of the clipped windows of the centres below the cap, and 1 for each capped centre
 *     [2] capped centres   [3] the largest clipped window of any centre, capped or not
 *   The maps do not depend on sq_out_dev or stats_dev being null.
 * How: a scatter.  The centres are compacted into a list (the exclusive scan of the mesh kernels; the list's length stays on the
 * device); each centre q walks its own window -- per axis the voxels within the largest k with fl((k s)^2) < rsq[q], clipped to the
 * volume: the bounding box of its ball, found exactly -- and, where d2 < rsq[q] and p is a centre, raises the 64-bit key of p to the bit
 * pattern of rsq[q] by an integer atomic max.  Positive doubles order like their bit patterns and a max is commutative and
 * associative, so these atomics cost no reproducibility: this is the one place where the QC kernels use an atomic on a result.  The
 * work is the sum of the centres' own windows ([1]), never the largest radius times the voxel count.
 * max_window_voxels (> 0) caps the clipped window of one centre: a centre above it scatters onto itself only and is counted in [2];
 * the map is then a lower bound, and the caller is told.  It guards shared machines against a blob that fills the volume (radius 80:
 * 10^13 tests), and is not an accuracy knob.  Every axis in [1, 32767] and D H W <= 2^31 - 1 (the list is int32), every spacing finite
 * and > 0.  The workspace holds the keys, the list, its scan and the centre bytes, 17 bytes per voxel.  Does not synchronise.
 * Known bias of the voxel radius: a slab t voxels thick along an axis of spacing s gets 2 ceil(t / 2) s at every voxel, between t s
 * and (t + 1) s; a sub-voxel radius (qc.local_thickness(radius="mesh")) removes it.
 *
 * oai_masked_stats: values_dev float32 [n]; mask_dev (may be null: every element) one byte per element, admitted where != 0.  An
 * element is counted when the mask admits it and its value is finite.  out_dev: double[8] on the device --
 *   [0] counted   [1] sum v   [2] sum v*v   [3] min   [4] max   [5], [6] the requested percentiles   [7] admitted non-finite values
 * With nothing counted [1]..[6] are NaN; a percentile slot that was not asked for is NaN.  The sums are fp64 sums of the widened
 * float32 values (v*v is exact there) in the fixed order of csrc/ordered_reduce.h, as oai_surface_distance: thread g of
 * min(2048, ceil(n / 1024)) blocks of 256 takes the elements g, g + threads, ... in that order, one slot per block, a one-block
 * finish.  The percentiles (n_percentiles = 0..2 host floats in [0, 100]) are np.percentile of the counted values as a float32 array,
 * to the bit: the radix select of csrc/radix_select.h with the ranks computed on the device, where alone the count is known.
 * n = 0 is allowed.  Does not synchronise.
 * ---------------------------------------------------------------------------------------- */
/* 0 when an axis is outside [1, 32767] or D*H*W > 2^31 - 1. */
size_t oai_local_thickness_workspace_bytes(int D, int H, int W);
int oai_local_thickness(const double* rsq_dev, int D, int H, int W, const double spacing_xyz[3], long long max_window_voxels,
                        double* sq_out_dev, float* thick_dev, void* workspace_dev, size_t workspace_bytes, long long* stats_dev, void* stream);
/* 0 when n < 0. */
size_t oai_masked_stats_workspace_bytes(long long n);
int oai_masked_stats(const float* values_dev, const unsigned char* mask_dev, long long n, const float* percentiles, int n_percentiles,
                     void* workspace_dev, size_t workspace_bytes, double* out_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Cartilage morphometry (csrc/morphometry.hip, tests/morphometry_ref.py): what reduces the per-vertex thickness on the atlas inner mesh
 * to per-knee figures -- mean thickness over the subchondral bone area, covered and denuded area, per region.  The reference has no
 * such step and VTK is absent: the definitions are this library's own, unpinned.  fp64 without contraction, every sum in a stated
 * order, no floating-point atomics: bit-reproducible.  With oai_point_footprint (above) these are its three primitives.
 *
 * oai_mesh_areas: verts_dev float32 [n_verts][3], faces_dev int32 [n_faces][3].  With a, b, c the corners of face f widened to double,
 *   e1 = b - a;  e2 = c - a;  cx = e1y*e2z - e1z*e2y;  cy = e1z*e2x - e1x*e2z;  cz = e1x*e2y - e1y*e2x
 *   face_area[f]   = 0.5 * sqrt((cx*cx + cy*cy) + cz*cz)
 *   vertex_area[v] = (sum of face_area[f] over the corners (f, k) that name v, in ascending 3 f + k) / 3.0
 * so a face that names a vertex twice counts twice for it (its area is 0), a vertex that no face names gets 0.0, and non-finite
 * coordinates propagate as IEEE gives them.  A face with an index outside [0, n_verts) has face_area NaN and is incident to no vertex.
 * face_area_dev float64 [n_faces] (may be null), vertex_area_dev float64 [n_verts].  The vertex-to-corner incidence is built by count,
 * exclusive scan and scatter (integer atomics for the slots); each vertex then adds its own corners smallest index first.  Does not
 * synchronise.  n_verts <= 2^31 - 2, n_faces <= 2^28.
 *
 * oai_region_stats: values_dev float32 [n], weights_dev float64 [n], labels_dev int32 [n] (may be null: every element in region 0),
 * covered_dev one byte per element (may be null: every element covered), 1 <= n_regions <= 64.  An element with a label outside
 * [0, n_regions) belongs to no region; it is MEASURED when it is covered (byte != 0) and its value is finite.  With t = (double)value
 * and w the weight, out_dev: double [n_regions][12] on the device, per region --
 *   [0] elements   [1] covered elements   [2] measured elements
 *   [3] sum w over all elements   [4] sum w over covered   [5] sum w over measured
 *   [6] sum w*t over measured   [7] sum (w*t)*t over measured   [8] min t   [9] max t over measured   [10] sum t   [11] sum t*t over measured
 * in the fixed order of csrc/ordered_reduce.h with oai_surface_distance's layout: thread g of max(1, min(2048, ceil(n / 1024))) blocks
 * of 256 takes the elements g, g + threads, ... in that order, one slot row per block and region, a one-block finish per region.  An
 * element outside a region performs no operation on that region's accumulator.  An empty region reads 0 for counts and sums, +inf
 * for the minimum and -inf for the maximum (+0 and -0 compare equal: which of them a minimum keeps is not specified).  n = 0 is
 * allowed.  Does not synchronise.
 * ---------------------------------------------------------------------------------------- */
/* 0 when n_verts is outside [0, 2^31 - 2] or n_faces outside [0, 2^28]. */
size_t oai_mesh_areas_workspace_bytes(long long n_verts, long long n_faces);
int oai_mesh_areas(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, void* workspace_dev, size_t workspace_bytes,
                   double* face_area_dev, double* vertex_area_dev, void* stream);
/* 0 when n < 0 or n_regions is outside [1, 64]. */
size_t oai_region_stats_workspace_bytes(long long n, int n_regions);
int oai_region_stats(const float* values_dev, const double* weights_dev, const int* labels_dev, const unsigned char* covered_dev, long long n,
                     int n_regions, void* workspace_dev, size_t workspace_bytes, double* out_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Mesh quality (csrc/mesh_quality.hip, tests/mesh_quality_ref.py): what can be asked of the surface that mesh-based thickness is measured
 * on -- is it closed and consistently oriented, does it fold through itself, how long is the inner / outer interface of a split, what
 * volume does it enclose.  The reference has no such step and VTK is absent: the definitions are this library's own, unpinned.  Every
 * integer is exact and does not depend on the order atomics land in; fp64 without contraction, every sum in a stated order, no
 * floating-point atomics: bit-reproducible.  verts_dev float32 [n_verts][3], faces_dev int32 [n_faces][3]; n_verts <= 2^31 - 2,
 * n_faces <= 2^28; n_faces = 0 is allowed and yields zeros.  None of the three synchronises or reads anything back.
 *
 * A face with an index outside [0, n_verts) is an argument error that only the device can see: oai_mesh_topology counts such faces in
 * record[14] (the caller refuses the mesh when it is not 0; mesh_processing.mesh_topology raises), and all three entry points read no
 * vertex through such a face: it has no edges, no area and meets nothing.
 *
 * oai_mesh_topology.  A face with two equal indices is DEGENERATE: counted, no edges.  Half-edge (f, k) runs from faces[f][k] to
 * faces[f][(k+1)%3]; an undirected edge is owned by its half-edge with the smallest 3 f + k.  With m the number of half-edges on an edge:
 *   1 boundary (m = 1)   2 manifold (m = 2, opposite directions)   3 misoriented (m = 2, same direction)   4 non-manifold (m >= 3)
 * side_dev (may be null): int8 per face, -1 / 0 / +1 as DeviceSplit.side; a manifold edge whose two faces have sides -1 and +1 is
 * additionally an INTERFACE edge.  edge_class_dev: uint8 [n_faces][3], 0 where the half-edge is not the owner (or the face has no edges),
 * otherwise the class, plus 16 on an interface edge.  record_dev: int64 [16] on the device --
 *   [0] faces   [1] degenerate faces   [2] referenced vertices (named by a face that has edges)   [3] edges
 *   [4] boundary   [5] misoriented   [6] non-manifold   [7] interface edges
 *   [8] faces of side -1   [9] of side 0   [10] of side +1 (all faces; 0 0 0 without side_dev)
 *   [11] Euler characteristic = [2] - [3] + ([0] - [1] - [14])
 *   [12] boundary loops = connected components of the graph of boundary edges   [13] interface loops, likewise
 *   [14] faces with an index outside the mesh   [15] manifold edges
 * A CSR of half-edges keyed by the edge's smaller vertex (count, exclusive scan, scatter), then each half-edge walks its vertex's list:
 * a vertex of valence v costs v^2 there, and nothing depends on the scatter order.  The loops are counted by one workgroup per edge set
 * with the hook / jump rounds of oai_mesh_components, run to convergence inside the kernel.
 *
 * oai_mesh_geometry: edge_class_dev as written by oai_mesh_topology for the same faces.  With a, b, c the corners of face f widened to
 * double and o = origin (host pointer, 3 doubles),
 *   area  A    = oai_mesh_areas' face_area
 *   l_k        = (dx*dx + dy*dy) + dz*dz of corner (k+1)%3 minus corner k;   edge length = sqrt(l_k)
 *   q          = (6.928203230275509 * A) / ((l_0 + l_1) + l_2), 0 where the denominator is not > 0   (4 sqrt 3 A / sum l: 1 equilateral, 0 flat)
 *   det(u,v,w) = (ux*(vy*wz - vz*wy) - uy*(vx*wz - vz*wx)) + uz*(vx*wy - vy*wx)   with u = a - o, v = b - o, w = c - o
 * record_dev: float64 [16] on the device --
 *   [0] surface area = sum A   [1] signed enclosed volume = (sum det) / 6.0 (positive for outward counter-clockwise faces of a closed mesh)
 *   [2] boundary length   [3] interface length   [4] min   [5] max   [6] mean edge length over owned edges (sum / count)
 *   [7] min   [8] max face area   [9] min q   [10] mean q (sum / faces)   [11] faces with q < q_min   [12] owned edges   [13] faces summed
 * Sums run over faces in the fixed order of csrc/ordered_reduce.h with oai_region_stats' layout (thread g of max(1, min(2048,
 * ceil(n_faces / 1024))) blocks of 256 takes the faces g, g + threads, ...; a face adds its figures, then its owned half-edges k = 0, 1, 2);
 * minima and maxima are fmin / fmax.  Degenerate faces take part (area 0, q 0).  Figures over an empty set read 0.
 *
 * oai_mesh_self_intersections.  orient(a,b,c,d) = det(b - a, c - a, d - a) with the expansion above on the widened corners.  The edge
 * pq PROPERLY PIERCES the triangle abc when orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs and orient(p,q,a,b),
 * orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0.  Faces f < g that share no vertex index INTERSECT when an edge (k, (k+1)%3) of
 * one properly pierces the other.  Two limits follow: coplanar overlap and mere touching are not seen (strict signs), and neither is a fold
 * between faces that share a vertex.  Broad phase: each face goes into every cell of the uniform grid (grid_lo, cell_size, grid_dims: host
 * pointers; cell = floor((x - lo) / cell_size) clamped to the grid) that its bounding box spans -- count, scan, scatter -- and a pair is
 * evaluated only in the cell that holds the lower corner of the two cell ranges' intersection, so once.  The result is the same for every
 * valid grid.  The entry list lives in the workspace, sized by `capacity` entries: when the faces need more, nothing is tested, flag is
 * all 0 and record[3] = 1.  flag_dev: uint8 [n_faces], 1 on a face of an intersecting pair.  record_dev: int64 [4] on the device --
 *   [0] intersecting pairs   [1] flagged faces   [2] bin entries needed   [3] overflow
 * ---------------------------------------------------------------------------------------- */
/* 0 when n_verts is outside [0, 2^31 - 2] or n_faces outside [0, 2^28]. */
size_t oai_mesh_topology_workspace_bytes(long long n_verts, long long n_faces);
int oai_mesh_topology(const int* faces_dev, long long n_faces, long long n_verts, const signed char* side_dev, void* workspace_dev,
                      size_t workspace_bytes, unsigned char* edge_class_dev, long long* record_dev, void* stream);
/* 0 when n_faces is outside [0, 2^28]. */
size_t oai_mesh_geometry_workspace_bytes(long long n_faces);
int oai_mesh_geometry(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, const unsigned char* edge_class_dev,
                      const double origin[3], double q_min, void* workspace_dev, size_t workspace_bytes, double* record_dev, void* stream);
/* 0 when n_faces is outside [0, 2^28], an axis of the grid is < 1, it has more than 2^31 - 2 cells or capacity is outside [0, 2^31 - 2]. */
size_t oai_mesh_self_intersections_workspace_bytes(long long n_faces, const int grid_dims[3], long long capacity);
int oai_mesh_self_intersections(const float* verts_dev, long long n_verts, const int* faces_dev, long long n_faces, const double grid_lo[3],
                                double cell_size, const int grid_dims[3], long long capacity, void* workspace_dev, size_t workspace_bytes,
                                unsigned char* flag_dev, long long* record_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Cohort statistics (csrc/group_stats.hip, tests/group_stats_ref.py): permutation tests on N per-knee vectors that share the atlas
 * inner vertices -- where do two groups of knees differ, where does a follow-up differ from baseline, with a family-wise error that
 * holds over the surface.  The reference has no such step: the definitions are this library's own, pinned by the numpy restatement and
 * scipy.  fp64 without contraction; EVERY SUM OVER KNEES RUNS IN ASCENDING KNEE INDEX WITH ONE ACCUMULATOR that starts at +0.0, and a
 * knee that does not take part adds +0.0; no floating-point atomics; counts are integers: bit-reproducible.  None of the four
 * synchronises or reads anything back.  2 <= n_knees <= 2^24, 1 <= n_verts <= 2^31 - 2, at most 2^20 rows per call.
 *
 * Layout.  y_dev float32 [n_knees][n_verts], knee-major.  mask_dev uint8 [n_knees][n_verts], non-zero = this knee has a value at this
 * vertex; may be null: every entry is valid.  bits_dev uint32 [P][ceil(n_knees / 32)]: knee i of row p is bit i % 32 of word i / 32.
 * Row 0 is the observed labelling by convention: oai_permutation_reduce treats the batch with p0 = 0 as the one that holds it.
 *
 * oai_group_prepare.  With m_i the mask and y_i = (double)y[i][v] where m_i, else 0.0 -- per vertex v, i = 0 .. n_knees - 1:
 *   n    = sum m_i                 mean = (sum y_i) / (double)n                   (n = 0: NaN)
 *   d_i  = y_i - mean where m_i, else 0.0
 *   c_i  = d_i when centre = 1 (two-sample: centring does not change the statistic under permutation and keeps Q - S*S/n well
 *          conditioned), y_i when centre = 0 (one-sample: the values are paired differences and their sign matters)
 *   q_i  = c_i * c_i               S = sum c_i      Q = sum q_i
 *   std  = sqrt((sum d_i * d_i) / (double)(n - 1)), NaN when n < 2: the descriptive figure, centred in both cases
 * A NaN under a non-zero mask byte propagates.  The results fill the PREPARED BLOCK, workspace_dev, front to back, each array starting
 * on the next multiple of 256 bytes: C float64 [n_knees][n_verts], Qm likewise, S, Q, mean, std float64 [n_verts], n int32 [n_verts].
 * oai_permutation_t reads the block; it stays valid for as long as the caller keeps it.
 *
 * oai_permutation_t: rows [p0, p1) of bits_dev -> the t tile, float64 [p1 - p0][n_verts] at the start of workspace_dev.  b_i = bit i.
 *   OAI_STATS_TWO_SAMPLE (prepared with centre = 1; bit = the knee is in group 1; mask_dev as given to oai_group_prepare):
 *     n1 = sum b_i & m_i           S1 = sum (b_i ? c_i : 0.0)     Q1 = sum (b_i ? q_i : 0.0)
 *     n2 = n - n1;  S2 = S - S1;  Q2 = Q - Q1
 *     ss  = (Q1 - S1*S1/n1) + (Q2 - S2*S2/n2)          (a*a/b is (a*a)/b)
 *     sp2 = ss / (n - 2)
 *     t   = (S1/n1 - S2/n2) / sqrt(sp2 * (1.0/n1 + 1.0/n2))        valid iff n1 >= 2 && n2 >= 2 && sp2 > 0, otherwise NaN
 *   Student's pooled t, the sign of mean(group 1) - mean(group 2).
 *   OAI_STATS_ONE_SAMPLE (prepared with centre = 0; bit = flip the sign of the knee; mask_dev is not read):
 *     Sf  = sum (b_i ? -c_i : c_i)
 *     var = (Q - Sf*Sf/n) / (n - 1)
 *     t   = (Sf/n) / sqrt(var/n)                                    valid iff n >= 2 && var > 0, otherwise NaN
 * A thread owns one vertex and sixteen rows; a wave64 covers 64 consecutive vertices, so a label word is wave-uniform.  The kernel
 * issues "s + (b ? c : 0.0)" as fma(c, b ? 1.0 : 0.0, s) and "s + (b ? -c : c)" as fma(c, b ? -1.0 : 1.0, s): the product is exact, so
 * these are the bits of the stated adds for every finite c (with a non-finite c the t is NaN on either route).
 *
 * oai_permutation_reduce: the tile of rows [p0, p1).  max_abs_dev float64 [P]: entry p = max |t| of row p over its non-NaN entries, 0.0
 * when it has none (an exact maximum: no order to state).  When p0 = 0, t0_dev float64 [n_verts] receives row 0 of the tile and
 * exceed_dev int64 [n_verts] is STARTED; otherwise t0_dev is read and exceed_dev added to:
 *   exceed[v] += number of rows p of the batch with |t_p(v)| >= |t_0(v)|, both not NaN        (row 0 counts itself)
 *
 * oai_graph_clusters: values_dev float64 [n_rows][n_verts] (any values: a t tile), the CSR vertex adjacency of oai_mesh_adjacency
 * (offsets_dev int32 [n_verts + 1], neighbours_dev int32 [n_neighbours]; an offset outside [0, n_neighbours] is clamped, a neighbour
 * outside [0, n_verts) is ignored), threshold t0 > 0.  Per row two vertex sets, {t > t0} and {t < -t0} (strict; NaN is in neither);
 * connected components within each set, so two adjacent vertices of opposite sign never join.  A component's label is its smallest
 * vertex index (as oai_label_components), a vertex in neither set has label -1 and size 0.  max_extent_dev int32 [n_rows]: the vertex
 * count of the row's largest component over both signs, 0 if none.  label0_dev, size0_dev int32 [n_verts] (each may be null): row 0's
 * labels and, per vertex, the size of its component.  One workgroup per row runs hook / jump rounds (oai_mesh_components) until a round
 * changes nothing; labels and sizes live in the workspace, so n_verts is not bounded by LDS.  Integers only.
 * ---------------------------------------------------------------------------------------- */
#define OAI_STATS_TWO_SAMPLE 0
#define OAI_STATS_ONE_SAMPLE 1
/* All four: 0 for a shape the entry point refuses. */
size_t oai_group_prepare_workspace_bytes(long long n_knees, long long n_verts);
int oai_group_prepare(const float* y_dev, const unsigned char* mask_dev, long long n_knees, long long n_verts, int centre, void* workspace_dev,
                      size_t workspace_bytes, void* stream);
size_t oai_permutation_t_workspace_bytes(long long n_rows, long long n_verts);
int oai_permutation_t(const void* prepared_dev, size_t prepared_bytes, const unsigned char* mask_dev, const unsigned* bits_dev, long long n_knees,
                      long long n_verts, long long p0, long long p1, int mode, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t oai_permutation_reduce_workspace_bytes(long long n_rows, long long n_verts);
int oai_permutation_reduce(const double* tile_dev, long long n_verts, long long p0, long long p1, void* workspace_dev, size_t workspace_bytes,
                           double* t0_dev, double* max_abs_dev, long long* exceed_dev, void* stream);
size_t oai_graph_clusters_workspace_bytes(long long n_rows, long long n_verts);
int oai_graph_clusters(const double* values_dev, long long n_rows, long long n_verts, const int* offsets_dev, const int* neighbours_dev,
                       long long n_neighbours, double t0, void* workspace_dev, size_t workspace_bytes, int* max_extent_dev, int* label0_dev,
                       int* size0_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Cohort regression (csrc/group_regression.hip, tests/group_regression_ref.py): how does thickness vary with one regressor of interest
 * x, vertex by vertex, adjusted for nuisance covariates -- the model y ~ Z gamma + x beta over the knees that have a value at the vertex,
 * the t of beta, and its null distribution under permutation.  Z has q nuisance columns, the intercept (if any) counted among them; the
 * design D = [Z | x] has p = q + 1 columns WITH x LAST, 1 <= p <= 6.  The permutation scheme is Freedman and Lane's, as recalled from
 * Winkler et al. 2014 (NeuroImage 92) and NOT pinned to any implementation: y is residualised on Z once, then the rows of the whole
 * design are permuted against the fixed residuals and their fixed mask -- algebraically the same as permuting the residuals, and it keeps
 * "missing" attached to the data.  The reference has no such step: the definitions are this library's own, pinned by the numpy
 * restatement and scipy.  The rules of "Cohort statistics" hold: fp64 without contraction, no floating-point atomics, one accumulator
 * per sum that starts at +0.0, EVERY SUM OVER KNEES IN ASCENDING KNEE INDEX: bit-reproducible.  Neither entry point synchronises or reads
 * anything back.  2 <= n_knees <= 2^24, 1 <= n_verts <= 2^31 - 2, at most 2^20 rows per call.  y_dev and mask_dev as in "Cohort
 * statistics"; nuisance_dev float64 [n_knees][q] and design_dev float64 [n_knees][p], knee-major; perm_dev int32 [P][n_knees].
 *
 * Cholesky, A = L L^T of a symmetric matrix given by its lower triangle, in this order: for a = 0 .. size-1 { s = A_aa;
 * for k < a ascending: s = s - L_ak*L_ak;  PIVOT RULE (a condition, not a measurement): pivot s is accepted iff s > 1e-10 * A_aa;
 * L_aa = sqrt(s);  for c = a+1 .. size-1 { s = A_ca; for k < a ascending: s = s - L_ck*L_ak;  L_ca = s / L_aa } }.  The arithmetic
 * goes on after a pivot that is not accepted; what it then leaves in R and Q is IEEE arithmetic like the rest.
 *
 * oai_regression_prepare.  With m_i and y_i as in oai_group_prepare -- per vertex v, i = 0 .. n_knees - 1:
 *   n    = sum m_i                 mean = (sum y_i) / (double)n
 *   d_i  = y_i - mean where m_i and centre = 1;  y_i where m_i and centre = 0;  0.0 otherwise
 *   q > 0:  A_ac = sum_i (m_i ? z_ia*z_ic : 0.0), c <= a       h_a = sum_i z_ia*d_i   (a product, then an add: two roundings)
 *           A = L L^T;  L w = h forward (w_a = (h_a - sum_{k<a} L_ak*w_k) / L_aa, s = s - L_ak*w_k, k ascending);
 *           L^T gamma = w backward, a = q-1 .. 0 (gamma_a = (w_a - sum_{k>a} L_ka*gamma_k) / L_aa, s = s - L_ka*gamma_k, k ascending)
 *           r_i = m_i ? d_i - sum_a z_ia*gamma_a : 0.0        (from d_i, s = s - z_ia*gamma_a, a ascending)
 *   q = 0:  r_i = d_i
 *   Q    = sum r_i*r_i
 *   ok   = every pivot of A accepted && n - p >= 1
 * The PREPARED BLOCK, prepared_dev, front to back, each array starting on the next multiple of 256 bytes: R float64 [n_knees][n_verts],
 * Q, mean float64 [n_verts], n int32 [n_verts], ok uint8 [n_verts].
 *
 * oai_regression_t: rows [p0, p1) of perm_dev -> the t tile, float64 [p1 - p0][n_verts] at the start of workspace_dev, which
 * oai_permutation_reduce and oai_graph_clusters consume as they are.  Knee j of row pi takes design row perm[pi][j]; an index outside
 * [0, n_knees) is clamped.  Row 0 is the identity by convention.  Per (row, vertex), g_j = D[perm[pi][j]] (p doubles), j ascending:
 *   M_ac = sum_j (m_j ? g_ja*g_jc : 0.0), c <= a             b_a = sum_j g_ja*r_j   (a product, then an add)
 *   M = L L^T, same order and pivot rule;   L z = b forward, as above
 *   rss = Q - sum_a z_a*z_a                 (from Q, s = s - z_a*z_a, a ascending)
 *   dof = n - p;   s2 = rss / (double)dof;   t = z_p / sqrt(s2)          (z_p: the last entry, that of x)
 *   valid iff ok[v] && every pivot of M accepted && dof >= 1 && s2 > 0, otherwise NaN
 * With p0 = 0 and slope0_dev (float64 [n_verts]) not null, row 0 also writes beta = z_p / L_pp there, NaN where its t is.
 * mask_dev as given to oai_regression_prepare; null: every entry is valid, and the results are THE SAME BITS as with a mask of all ones.
 * A thread owns one vertex and R rows (R depends on p and on whether there is a mask).  The product g_ja*g_jc is formed once, in fp64,
 * by a gather kernel that writes the batch's permuted design into the workspace; the t kernel issues "M + (m ? G : 0.0)" as
 * fma(G, m ? 1.0 : 0.0, M): the product is exact, so these are the bits of the stated add for every finite design.  Without a mask M
 * and L do not depend on the vertex and are formed once per row, in the same order.
 * ---------------------------------------------------------------------------------------- */
/* Both: 0 for a shape the entry point refuses. */
size_t oai_regression_prepare_workspace_bytes(long long n_knees, long long n_verts);
int oai_regression_prepare(const float* y_dev, const unsigned char* mask_dev, const double* nuisance_dev, long long n_knees, long long n_verts,
                           int n_nuisance, int centre, void* prepared_dev, size_t prepared_bytes, void* stream);
size_t oai_regression_t_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns);
int oai_regression_t(const void* prepared_dev, size_t prepared_bytes, const unsigned char* mask_dev, const double* design_dev, const int* perm_dev,
                     long long n_knees, long long n_verts, int n_columns, long long p0, long long p1, void* workspace_dev, size_t workspace_bytes,
                     double* slope0_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Cohort F test (csrc/group_regression.hip, tests/group_f_ref.py): do SEVERAL design columns explain thickness jointly, vertex by
 * vertex, adjusted for the columns before them -- a one-way ANOVA over a factor with k + 1 levels (k dummy columns), an interaction
 * together with its main effect, a quadratic term with the linear one.  The design is D = [Z | X] with p = n_columns columns,
 * 1 <= p <= 6, of which THE k = n_interest COLUMNS OF INTEREST COME LAST, 1 <= k <= p; the first q = p - k columns are nuisance, the
 * intercept (if any) among them.  Everything that is not restated here is as in "Cohort regression": Freedman and Lane's permutation
 * of the design rows against the residuals (Winkler et al. 2014, as recalled, NOT pinned to any implementation), the layouts, the
 * clamping of an index outside [0, n_knees), row 0 the identity by convention, the limits on knees, vertices and rows, fp64 without
 * contraction, no floating-point atomics, one accumulator per sum that starts at +0.0, EVERY SUM OVER KNEES IN ASCENDING KNEE INDEX:
 * bit-reproducible.  Nothing synchronises or reads anything back.  The definitions are this library's own, pinned by the numpy
 * restatement and, through it, scipy's one-way F and numpy's least squares.
 *
 * prepared_dev is the block of oai_regression_prepare called with n_nuisance = q = n_columns - n_interest, an entry point that is used
 * as it is.  THE CALLER IS RESPONSIBLE FOR HAVING PREPARED WITH THE MATCHING q: the block does not record it and oai_regression_f
 * cannot check it.  Its ok only guarantees n - (q + 1) >= 1, so oai_regression_f applies its own dof >= 1, as oai_regression_t does.
 *
 * oai_regression_f: rows [p0, p1) of perm_dev -> the F tile, float64 [p1 - p0][n_verts] at the start of workspace_dev (the workspace is
 * laid out as oai_regression_t's: the tile, then the table, then the factors, and the size is the same).  F >= 0, so
 * oai_permutation_reduce (max |.| and exceedance counts), oai_graph_clusters and oai_graph_tfce take the tile as it is.  Per (row,
 * vertex):
 *   M, b, L, z   as in oai_regression_t
 *   rss = Q - sum_a z_a*z_a                        (from Q, s = s - z_a*z_a, a = 0 .. p-1 ascending)
 *   ess = sum_{a=q}^{p-1} z_a*z_a                  (from +0.0, s = s + z_a*z_a, a ascending)
 *   dof = n - p;  s2 = rss / (double)dof;  F = (ess / (double)k) / s2
 *   valid iff ok[v] && every pivot of M accepted && dof >= 1 && s2 > 0, otherwise NaN
 * ess is the extra sum of squares that the last k columns explain given the first q: L z = b orthogonalises the columns in their
 * order.  With k = 1, F is the square of oai_regression_t's t up to rounding (z_p*z_p / s2 against (z_p / sqrt(s2))^2).
 * With p0 = 0 and coef0_dev (float64 [k][n_verts]) not null, row 0 also writes the coefficients of the columns of interest there, entry
 * a - q for column a, NaN where its F is NaN -- back substitution on the trailing block of L:
 *   for a = p-1 down to q { s = z_a;  for j = a+1 .. p-1 ascending: s = s - L_ja*beta_j;  beta_a = s / L_aa }
 * A later batch (p0 > 0) leaves coef0_dev alone.  mask_dev as given to oai_regression_prepare; null: every entry is valid, and the
 * results are THE SAME BITS as with a mask of all ones.  The kernel is oai_regression_t's with another epilogue: same rows per thread,
 * same gather and row-factor kernels, the same fma(G, m ? 1.0 : 0.0, M) for the stated add.
 * ---------------------------------------------------------------------------------------- */
/* 0 for a shape the entry point refuses; equal to oai_regression_t_workspace_bytes otherwise. */
size_t oai_regression_f_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns);
int oai_regression_f(const void* prepared_dev, size_t prepared_bytes, const unsigned char* mask_dev, const double* design_dev, const int* perm_dev,
                     long long n_knees, long long n_verts, int n_columns, int n_interest, long long p0, long long p1, void* workspace_dev,
                     size_t workspace_bytes, double* coef0_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Vertex-wise design columns (csrc/group_regression_vx.hip, tests/vertex_regression_ref.py): the models of "Cohort regression" and
 * "Cohort F test" in which S = 1 or 2 of the design columns are MAPS on the atlas -- one number per (knee, vertex) and not one per
 * knee: baseline thickness at the same vertex as the adjustment of a rate of change (regression to the mean), the normative z-score or
 * the previous visit at the vertex as the regressor.  FSL randomise has such columns as voxel-wise EVs and PALM as -evperdat, AS
 * RECALLED and NOT pinned to any implementation; the reference has no such step: the definitions are this library's own, pinned by the
 * numpy restatement and, through it, numpy's least squares.  Everything that is not restated here is as in "Cohort regression" and
 * "Cohort F test": Freedman and Lane's permutation of the design rows against the residuals, fp64 without contraction, no
 * floating-point atomics, one accumulator per sum that starts at +0.0, EVERY SUM OVER KNEES IN ASCENDING KNEE INDEX, the Cholesky order
 * and the PIVOT RULE s > 1e-10 * A_aa, the clamping of an index outside [0, n_knees), row 0 the identity by convention, the limits on
 * knees, vertices and rows.  Nothing synchronises or reads anything back.
 *
 * THE DESIGN AT VERTEX v has p <= 6 columns IN THIS ORDER: [ vertex nuisance (s_n) | global nuisance (q_g) | global interest (k_g) |
 * vertex interest (s_i) ], with S = s_n + s_i in {1, 2}, s_i in {0, 1}, and s_i = 1 only with k_g = 0: the per-vertex column is then the
 * one regressor of interest.  The intercept, if any, is among the global nuisance columns.  The per-vertex nuisance columns come first
 * so that their position is a compile-time constant; the order of nuisance columns changes no statistic mathematically and is part of
 * the bit contract.
 *
 * Inputs.  y_dev float32 and mask_dev uint8 [n_knees][n_verts] as in "Cohort regression" (mask_dev null: every entry is valid).  w_dev
 * float32 [S][n_knees][n_verts], the per-vertex columns in the design's order; wmask_dev uint8 [S][n_knees][n_verts], or null: every
 * entry is valid.  nuisance_dev float64 [n_knees][q_g]; global_dev float64 [n_knees][q_g + k_g], the global columns in the design's
 * order; perm_dev int32 [P][n_knees].
 *
 * oai_regression_vx_prepare.  Per vertex v, with my_i the validity of y and mw_si that of column s at knee i, every sum in ascending i:
 *   m_i  = my_i && mw_0i (&& mw_1i)           the EFFECTIVE MASK: complete cases
 *   n    = sum m_i            n_dropped = sum (my_i && !m_i)
 *   wbar_s = (sum_{m_i} (double)w_si) / (double)n            per column s
 *   wc_si  = (double)w_si - c where mw_si (valid at that knee in its own right), otherwise wbar_s - c;  c = wbar_s if centre, else 0.0
 *            THE COMPLETED VALUE: a missing covariate entry sits on the complete-case mean, and a centred missing entry is exactly 0.0
 *            (a select, not a subtraction).  With n = 0 every wc is 0.0.
 *   mean, d_i, A, h, gamma, r_i, Q, ok   as oai_regression_prepare states them, over the q = s_n + q_g nuisance columns
 *            z_i = [wc_0i .. | nuisance_i ..], with the effective mask standing in for m; a product with a per-vertex entry is one
 *            rounding, then the add.
 * The prepared block is that of "Cohort regression" (R, Q, mean, n, ok) followed by n_dropped int32 [n_verts], the effective mask uint8
 * [n_knees][n_verts] and WC float64 [S][n_knees][n_verts], each array starting on the next multiple of 256 bytes.
 *
 * oai_regression_vx_t and oai_regression_vx_f: rows [p0, p1) of perm_dev -> the tile, float64 [p1 - p0][n_verts] at the start of
 * workspace_dev, which oai_permutation_reduce, oai_graph_clusters and oai_graph_tfce take as it is.  KNEE j OF ROW pi TAKES THE WHOLE
 * DESIGN ROW perm[pi][j]: the global entries of that knee, and WC[s][perm[pi][j]][v] for the per-vertex ones.  Missingness stays
 * attached to the data: entry j counts iff the effective m_j, whichever row it is dealt; a dealt row whose own covariate was missing
 * contributes its completed value.  UNDER THE IDENTITY ROW a completed value never enters a sum with a non-zero weight (m_j is 0 and r_j
 * is 0.0 there), so the observed statistic is the exact complete-case fit; only the null distribution sees the mean-imputed entries.
 * n, dof = n - p and Q do not depend on the row.  Per (row, vertex), g_j the dealt design row (p doubles), j ascending:
 *   M_ac = sum_j (m_j ? g_ja*g_jc : 0.0), c <= a     the product rounded once; global x global products are formed once per batch by a
 *          gather kernel, a product with a per-vertex factor is formed in the thread; either way the add is issued as
 *          fma(prod, m ? 1.0 : 0.0, M), which gives the bits of the stated add for every finite design
 *   b_a  = sum_j g_ja*r_j                            (a product, then an add)
 *   L, z, rss, dof, s2, t, F, ess, validity, slope0 and coef0 exactly as oai_regression_t and oai_regression_f state them; t is that of
 *   the LAST column (the per-vertex one when s_i = 1), F that of the last k = n_interest columns, which are global (s_i = 0).
 * There is no unmasked fast path: M depends on the vertex.  A null mask_dev together with a null wmask_dev gives THE SAME BITS as masks
 * of all ones.  The result does not depend on the rows per thread or on the batch; a later batch (p0 > 0) leaves slope0_dev / coef0_dev
 * alone.  THE CALLER IS RESPONSIBLE FOR HAVING PREPARED WITH THE MATCHING s_n, s_i and q_g = n_columns - S - (k_g).
 * Refused, with a status and a message that names the entry point, before anything is launched: null pointers, n_columns outside
 * [1, 6], S outside {1, 2}, s_i = 1 with n_interest > 0, n_interest < 1 for F, no column of interest left for t, bad row ranges, a short
 * workspace or prepared block.
 * ---------------------------------------------------------------------------------------- */
/* All three: 0 for a shape the entry point refuses. */
size_t oai_regression_vx_prepare_workspace_bytes(long long n_knees, long long n_verts, int n_vertex_columns);
int oai_regression_vx_prepare(const float* y_dev, const unsigned char* mask_dev, const float* w_dev, const unsigned char* wmask_dev,
                              const double* nuisance_dev, long long n_knees, long long n_verts, int n_vertex_nuisance, int n_vertex_interest,
                              int n_global_nuisance, int centre, void* prepared_dev, size_t prepared_bytes, void* stream);
size_t oai_regression_vx_t_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns, int n_vertex_columns);
int oai_regression_vx_t(const void* prepared_dev, size_t prepared_bytes, const double* global_dev, const int* perm_dev, long long n_knees,
                        long long n_verts, int n_columns, int n_vertex_nuisance, int n_vertex_interest, long long p0, long long p1, void* workspace_dev,
                        size_t workspace_bytes, double* slope0_dev, void* stream);
size_t oai_regression_vx_f_workspace_bytes(long long n_rows, long long n_verts, long long n_knees, int n_columns, int n_vertex_columns);
int oai_regression_vx_f(const void* prepared_dev, size_t prepared_bytes, const double* global_dev, const int* perm_dev, long long n_knees,
                        long long n_verts, int n_columns, int n_vertex_nuisance, int n_vertex_interest, int n_interest, long long p0, long long p1,
                        void* workspace_dev, size_t workspace_bytes, double* coef0_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Cluster-robust regression (csrc/cluster_robust.hip, tests/cluster_robust_ref.py): the model of "Cohort regression" for rows that are
 * NOT exchangeable because they come in clusters -- the visits of a subject in a longitudinal cohort, both knees of a subject in a
 * cross-sectional one.  The marginal model: ordinary least squares over all rows, a cluster-robust (sandwich) variance that sums the
 * scores within a cluster (Liang and Zeger 1986), and inference from the restricted wild cluster bootstrap, which flips the sign of
 * every cluster's null-model residuals as a block (Cameron, Gelbach and Miller 2008; Guillaume et al. 2014 for longitudinal images) --
 * all AS RECALLED and NOT pinned to any implementation.  The reference has no such step: the definitions are this library's own, pinned
 * by the numpy restatement and, through it, numpy's least squares and the explicit sandwich.  The rules of "Cohort regression" hold:
 * fp64 without contraction, no floating-point atomics, one accumulator per sum that starts at +0.0, EVERY SUM OVER ROWS AND OVER
 * CLUSTERS IN ASCENDING INDEX, the Cholesky order, the solves and the PIVOT RULE s > 1e-10 * A_aa: bit-reproducible.  Neither entry
 * point synchronises or reads anything back.
 *
 * Rows are knee-visits in CLUSTER-MAJOR ORDER: cluster s owns rows offsets[s] .. offsets[s+1]-1 of offsets_dev int32 [n_clusters + 1];
 * an offset outside [0, n_rows] is clamped.  design_dev float64 [n_rows][p], THE REGRESSOR OF INTEREST IS THE LAST COLUMN, 1 <= p <= 6,
 * q = p - 1.  mask_dev uint8 [n_rows][n_verts] as in "Cohort statistics", or null.  2 <= n_clusters <= n_rows <= 2^20, 1 <= n_verts <=
 * 2^31 - 2, at most 2^20 flip rows per call.
 *
 * oai_cluster_prepare.  prepared_dev ALREADY HOLDS, at its front, the block of oai_regression_prepare called on the same rows with
 * n_knees = n_rows, the first q design columns as nuisance_dev and the same mask_dev: r, Q, n and ok are its.  THE CALLER IS RESPONSIBLE
 * for that call; the block does not record it.  Per vertex, with m_j the validity of row j:
 *   M_ac = Σ_j (m_j ? d_ja·d_jc : 0.0), j ascending.  M = L Lᵀ.
 *   a = M⁻¹ e_p.  Forward-solve L z = e_p, then back-solve Lᵀ a = z.
 *   w_j = m_j ? Σ_c d_jc·a_c : 0.0, c ascending.            (from +0.0, s = s + d_jc*a_c: a product, then an add)
 *   per cluster s, rows ascending:
 *     h_sc = Σ (m_j ? d_jc·r_j : 0.0)
 *     k_sc = Σ (m_j ? w_j·d_jc : 0.0)
 *     u_s = Σ (m_j ? w_j·r_j : 0.0)
 *     present_s = any m_j
 *   G = Σ_s present_s.
 *   c = (G/(G−1)) · ((n−1)/(n−p)), each quotient taken in double, then one product.  This is Stata's CR1.
 *   okc = ok && every pivot of M accepted && G ≥ 2 && n − p ≥ 1.
 * A cluster with no valid row at the vertex holds +0.0 throughout and adds +0.0.  With n − p = 0 or G = 1, c is what IEEE division
 * gives, and okc is 0.
 * THE CLUSTER BLOCK, prepared_dev, front to back, each array starting on the next multiple of 256 bytes: the block of "Cohort
 * regression" (R float64 [n_rows][n_verts], Q, mean float64 [n_verts], n int32 [n_verts], ok uint8 [n_verts]), then H float64
 * [p][n_clusters][n_verts], K float64 [p][n_clusters][n_verts], U float64 [n_clusters][n_verts], L float64 [p (p + 1) / 2][n_verts]
 * (entry (a, c), c <= a, in plane a (a + 1) / 2 + c), c float64 [n_verts], G int32 [n_verts], okc uint8 [n_verts] -- every plane
 * [.][n_clusters][n_verts], so that a read over v is coalesced -- and last the scratch of the unmasked path: float64 [n_rows], [p]
 * [n_clusters] and [p (p + 1) / 2 + 1 + p].  (2 p + 1) * n_clusters * n_verts * 8 bytes beside the regression block.
 * With mask_dev == NULL the quantities M, L, a, w and k do not depend on the vertex: they are formed once, in the same order, and
 * copied into the planes; the results are THE SAME BITS as with a mask of all ones.
 *
 * oai_cluster_t: rows [p0, p1) of bits_dev -> the t tile, float64 [p1 - p0][n_verts] at the start of workspace_dev, which
 * oai_permutation_reduce, oai_graph_clusters and oai_graph_tfce take as it is.  bits_dev uint32 [P][ceil(n_clusters / 32)], packed as in
 * "Cohort statistics" with CLUSTERS in the place of knees: f_s = −1 where bit s of the row is set and +1 otherwise.  Row 0 carries no
 * flips by convention.  Per (resample row π, vertex):
 *   1. b_c = Σ_s (bit ? −h_sc : h_sc), s ascending.  The negation is exact.  Then forward-solve L z = b and back-solve Lᵀ β = z.
 *   2. For s ascending: e = bit ? −u_s : u_s.  For c ascending, e = e − k_sc·β_c.  Then W = W + e·e.
 *   3. t = β_p / sqrt(c·W).  It is valid iff okc && W > 0, otherwise NaN.
 * (each k_sc·β_c a product, then the subtraction; e·e a product, then the add; c·W one product.)  Row 0 is the classical cluster-robust
 * t of the full model, by Frisch-Waugh: with p0 = 0 it also writes slope0 = β_p and se0 = sqrt(c·W) (float64 [n_verts], each may be
 * null), NaN where its t is; a later batch (p0 > 0) leaves both alone.  This is algebraically the restricted wild cluster bootstrap
 * y* = Z gamma~ + f o r~ refitted with the full model and its sandwich taken; the one-pass expansion of W into fixed quadratic terms
 * cancels and is NOT part of the contract.
 * A thread owns one vertex and R rows (R depends on p); the flip words are wave-uniform and come through scalar loads; "b + (bit ? -h :
 * h)" is issued as fma(h, bit ? -1.0 : 1.0, b) and the first step of e as fma(u, bit ? -1.0 : 1.0, -(k_s0*beta_0)): the products are
 * exact, so these are the bits of the stated operations for every finite value.  The result does not depend on R or on the batch.
 * Refused, with a status and a message that names the entry point, before anything is launched: n_clusters < 2, n_columns outside
 * [1, 6], more than 2^20 rows, n_rows < n_clusters, null pointers, bad flip-row ranges, a short workspace or cluster block.
 * ---------------------------------------------------------------------------------------- */
/* Both sizes: 0 for a shape the entry point refuses. */
size_t oai_cluster_prepare_workspace_bytes(long long n_rows, long long n_verts, long long n_clusters, int n_columns);
int oai_cluster_prepare(const unsigned char* mask_dev, const double* design_dev, const int* offsets_dev, long long n_rows, long long n_verts,
                        long long n_clusters, int n_columns, void* prepared_dev, size_t prepared_bytes, void* stream);
size_t oai_cluster_t_workspace_bytes(long long n_rows, long long n_verts);
int oai_cluster_t(const void* prepared_dev, size_t prepared_bytes, const unsigned* bits_dev, long long n_rows, long long n_verts,
                  long long n_clusters, int n_columns, long long p0, long long p1, void* workspace_dev, size_t workspace_bytes,
                  double* slope0_dev, double* se0_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Threshold-free cluster enhancement (csrc/graph_tfce.hip, tests/graph_tfce_ref.py): a t tile in, a tile of the same shape out in which
 * every vertex holds the integral, over all thresholds h at or below its |t|, of extent(h)^E * h^H -- extent(h) being the size of the
 * vertex' connected component of {|t| >= h} on the surface.  It takes the place of a hand-picked cluster threshold: the family-wise p
 * comes from the permutation distribution of the row maximum, which oai_permutation_reduce forms from the TFCE tile as it does from a t
 * tile.  The scheme is Smith and Nichols' (NeuroImage 44, 2009), with PALM's surface setting (E = 1, H = 2, extent as area) as the
 * default, AS RECALLED and NOT pinned to any implementation: the definition below is this library's own, pinned by the brute-force numpy
 * restatement, which runs scipy's connected components from scratch at every level.  Its limits: the integral is a right-endpoint sum
 * with a FIXED step dh; E is 1/2 or 1 and H is 1 or 2; the sum stops at max_steps levels and reports what it cut.  The rules of "Cohort
 * statistics" hold: fp64 without contraction, no floating-point atomics, one accumulator per sum that starts at +0.0: bit-reproducible.
 * The entry point does not synchronise and reads nothing back.  1 <= n_rows <= 2^20, 1 <= n_verts <= 2^31 - 2.
 *
 * Inputs.  values_dev float64 [n_rows][n_verts]; the CSR adjacency as in oai_graph_clusters (an offset outside [0, n_neighbours] is
 * clamped, a neighbour outside [0, n_verts) is ignored).  weight_dev int64 [n_verts], each >= 0, or null: every weight is 1; the caller
 * guarantees sum(weight) < 2^53.  unit > 0: what one unit of weight is worth (1 for vertex counts, 2^-20 mm^2 for areas in 2^-20 mm^2).
 * dh finite and > 0.  e_mode OAI_TFCE_E_HALF | OAI_TFCE_E_ONE, h_mode OAI_TFCE_H_ONE | OAI_TFCE_H_TWO.  1 <= max_steps <= 65536.
 * tfce_dev must not overlap values_dev.
 *
 * Per row and vertex v, with t = values[row][v]:
 *   a = |t|;  side = +1 if t > 0, -1 if t < 0, 0 for +-0 and NaN
 *   h_k = (double)k * dh, k = 1 .. max_steps                 (one multiplication: h_k does not decrease with k)
 *   v is ACTIVE AT LEVEL k iff side != 0 and a >= h_k         (not strict; NaN is never active, +-inf is at every level)
 *   at level k the graph keeps an edge u - v iff both ends are active and of the same side: adjacent vertices of opposite sign never join
 *   W_k(v) = the int64 sum of the weights of v's component at level k     (an integer sum: no order to state)
 *   e = (double)W_k(v) * unit;   eE = e (E = 1) or sqrt(e) (E = 1/2);   hH = h_k (H = 1) or h_k * h_k (H = 2);   c_k = (eE * hH) * dh
 *   K(v) = the largest k <= max_steps at which v is active, 0 if there is none
 *   acc = +0.0;  acc = acc + c_k for k = K(v) down to 1       (DESCENDING: the order is part of the contract.  Components only grow as
 *                                                              the threshold falls, so one union-find per row serves every level.)
 *   tfce(v) = NaN where t is NaN;  acc where side >= 0;  -acc where side < 0  (so -0.0 for a negative t below dh)
 * clipped_dev int32 [n_rows]: the vertices of the row with a >= (double)(max_steps + 1) * dh, whose integral was cut; infinities count.
 * One workgroup per row; parent, level and component weight live in the workspace, so n_verts is not bounded by LDS.
 * ---------------------------------------------------------------------------------------- */
#define OAI_TFCE_E_HALF 0
#define OAI_TFCE_E_ONE 1
#define OAI_TFCE_H_ONE 0
#define OAI_TFCE_H_TWO 1
/* 0 for a shape the entry point refuses. */
size_t oai_graph_tfce_workspace_bytes(long long n_rows, long long n_verts);
int oai_graph_tfce(const double* values_dev, long long n_rows, long long n_verts, const int* offsets_dev, const int* neighbours_dev,
                   long long n_neighbours, const long long* weight_dev, double unit, double dh, int e_mode, int h_mode, int max_steps,
                   void* workspace_dev, size_t workspace_bytes, double* tfce_dev, int* clipped_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Surface smoothing (csrc/graph_smooth.hip, tests/graph_smooth_ref.py): every row of a float64 tile -- one knee's scalar field on the
 * atlas vertices -- is smoothed ALONG THE SURFACE by K sweeps of normalised neighbourhood averaging on a weighted vertex graph, the
 * step a study takes before the tests above so that its maps have a stated FWHM.  Entries may be MISSING: a validity mask travels with
 * the values, a missing entry is never read into a sum and (in keep mode) never invented, so the operator is a normalised average whose
 * denominator depends on row and vertex, not one fixed sparse matrix power.  Iterated nearest-neighbour averaging as an approximation
 * of the heat kernel on a surface is common practice in surface-based analysis AS RECALLED; the definition below is this library's own
 * and is pinned to no implementation, only to the numpy restatement.  Its limits: weights are the caller's (finite and >= 0: the
 * caller's guarantee, the device does not check it); distances along edges, not geodesics; what FWHM K sweeps amount to is the caller's
 * calibration (oai_analysis_2_amd.stats.sweeps_for_fwhm).  The rules of "Cohort statistics" hold: fp64 without contraction (every
 * product is rounded before it is added), no floating-point atomics, one accumulator per sum that starts at +0.0: bit-reproducible and
 * independent of the launch geometry.  The entry point launches all sweeps on the given stream itself (plain launches), does not
 * synchronise and reads nothing back.  1 <= n_rows <= 2^20, 1 <= n_verts <= 2^31 - 2.
 *
 * Inputs.  values_dev float64 [n_rows][n_verts]; mask_dev uint8 [n_rows][n_verts], non-zero = valid, or null: every entry is valid.
 * The CSR adjacency as in oai_graph_clusters (an offset outside [0, n_neighbours] is clamped, a neighbour outside [0, n_verts) is
 * ignored; a vertex listed among its own neighbours is a neighbour like any other).  edge_weight_dev float64 [n_neighbours], aligned
 * with neighbours_dev: entry e is the weight w_e with which the vertex that owns slot e reads neighbour nbr[e]; w_ij and w_ji may
 * differ.  self_weight_dev float64 [n_verts], or null: every self weight is 1.0.  1 <= sweeps <= 4096.  fill 0 (keep) or 1 (fill).
 *
 * One sweep, for every row and vertex i, reads (x_s, m_s) and writes (x_s+1, m_s+1); (x_0, m_0) are the inputs:
 *   num = +0.0;  den = +0.0
 *   if m_s[i]:                                     num = num + self_w[i] * x_s[i];   den = den + self_w[i]
 *   for e = off[i] .. off[i+1] - 1 ascending, j = nbr[e], if m_s[j]:
 *                                                  num = num + w[e] * x_s[j];        den = den + w[e]
 *   ok = (fill ? 1 : m_s[i]) && den > 0
 *   x_s+1[i] = ok ? num / den : +0.0;              m_s+1[i] = ok
 * An invalid entry is skipped by a select, never multiplied by 0: a NaN, an infinity or anything else stored under a 0 mask byte
 * reaches no sum.  What is stored at a VALID entry propagates as IEEE says (a valid NaN spreads one ring per sweep).  Keep mode: a
 * missing entry stays missing and gives nothing; a valid entry whose self weight and valid neighbours' weights sum to 0 drops out.  Fill
 * mode: a missing entry with a valid neighbour of positive weight becomes valid, so the valid set grows by one ring per sweep.
 * out_values_dev float64 [n_rows][n_verts] receives x_K, +0.0 where m_K is 0; out_mask_dev uint8 [n_rows][n_verts] receives m_K as 0 / 1
 * and may be null.  out_values_dev may be values_dev and out_mask_dev may be mask_dev: the inputs are consumed before the outputs are
 * written.  The workspace holds the tile transposed to [n_verts][n_rows] twice over (values and masks, ping and pong), so that the
 * gather of a neighbour is a contiguous run over rows: 2 * (8 + 1) bytes per entry.
 * ---------------------------------------------------------------------------------------- */
/* 0 for a shape the entry point refuses. */
size_t oai_graph_smooth_workspace_bytes(long long n_rows, long long n_verts);
int oai_graph_smooth(const double* values_dev, const unsigned char* mask_dev, long long n_rows, long long n_verts, const int* offsets_dev,
                     const int* neighbours_dev, long long n_neighbours, const double* edge_weight_dev, const double* self_weight_dev, int sweeps,
                     int fill, void* workspace_dev, size_t workspace_bytes, double* out_values_dev, unsigned char* out_mask_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Longitudinal change (csrc/visit_slopes.hip, tests/visit_slopes_ref.py): stage one of the two-stage (summary-measures) analysis of a
 * longitudinal study.  Every SUBJECT (one knee followed over time) has several VISITS, each a row of the visit matrix with a time in
 * years; per (subject, vertex) a straight line is fitted by least squares through the visits that have a value at that vertex, and its
 * slope -- mm per year -- is the map that stage two tests across subjects like any other ("Cohort statistics" and after).  Visits may
 * be unevenly spaced, a subject may miss a visit, and a vertex may be missing in some of a subject's visits: the fit at a vertex uses
 * what is valid THERE, so n, the mean time and the span differ from vertex to vertex.  Fitting a line per subject and carrying the
 * slopes forward is the summary-measures approach; FreeSurfer's long_mris_slopes does it for cortical thickness and names the measures
 * rate, avg, pc1 and spc AS RECALLED; the definition below is this library's own and is pinned to no implementation, only to the numpy
 * restatement, scipy.stats.linregress and numpy.polyfit.  The rules of "Cohort statistics" hold: fp64 without contraction (every
 * product is rounded before it is added), one accumulator per sum that starts at +0.0, THE SLOTS OF A SUBJECT IN ASCENDING CSR
 * POSITION, no floating-point atomics: bit-reproducible and independent of the launch geometry.  The entry point launches on the given
 * stream, does not synchronise and reads nothing back.  1 <= n_rows <= 2^24, 1 <= n_verts <= 2^31 - 2, 1 <= n_subjects <= 2^24,
 * 0 <= n_visits <= 2^24.
 *
 * Inputs.  values_dev float32 [n_rows][n_verts], the visit matrix: every row is one knee at one visit, in any order.  mask_dev uint8
 * [n_rows][n_verts], non-zero = valid, or null: every entry is valid.  subject_offsets_dev int32 [n_subjects + 1]: subject s owns the
 * CSR slots off[s] .. off[s+1] - 1; an offset outside [0, n_visits] is clamped.  visit_row_dev int32 [n_visits]: the row of values_dev
 * of each slot; a slot whose row is outside [0, n_rows) is skipped as if it were missing at every vertex.  visit_time_dev float64
 * [n_visits]: the time of each slot in years (finite: the caller's guarantee, the device does not check it).  reference_time_dev float64
 * [n_subjects]: the time at which fit_ref is evaluated, typically the subject's first visit.  min_visits >= 2.  min_span >= 0, finite.
 *
 * For subject s and vertex v, over the slots e of s that are valid at v, t_e = time[e], y_e = values[row[e]][v]:
 *   pass 1:  n = count;  St = St + t_e;  Sy = Sy + (double)y_e;  tmin, tmax over the valid slots
 *            tb = St / n;  yb = Sy / n
 *   pass 2:  dt = t_e - tb;  dy = (double)y_e - yb;  Sxx = Sxx + dt*dt;  Sxy = Sxy + dt*dy
 *            ok = n >= min_visits && Sxx > 0 && (tmax - tmin) >= min_span
 *            rate = Sxy / Sxx
 *   pass 3:  r = dy - rate*dt;  rss = rss + r*r
 *            avg = yb;  fit_ref = yb + rate * (tref_s - tb)
 *            resid_sd = n >= 3 ? sqrt(rss / (double)(n - 2)) : NaN
 * Sums centred on the means of pass 1: no cancelling formula.  A slot that is not valid at v is skipped by a select, never multiplied
 * by 0: a NaN, an infinity or anything else stored under a 0 mask byte reaches no sum.  What is stored at a VALID entry propagates as
 * IEEE says.  Two visits at the same time give Sxx = 0 and no slope; so does one visit, or none.
 *
 * Outputs, every one nullable and [n_subjects][n_verts]: rate_dev, avg_dev, fit_ref_dev, resid_sd_dev float64; n_dev int32, ALWAYS the
 * count, also where ok is false; out_mask_dev uint8, ok as 0 or 1.  Where ok is false the float outputs hold +0.0.  resid_sd holds NaN
 * exactly where ok is true and n == 2: two points have no residual.  A null output is neither computed nor written beyond what the
 * others need: pass 3 runs for resid_sd_dev alone.  The workspace holds the slot table that the first launch writes: per subject its
 * clamped slot run (two int32), per slot its row or -1.
 * ---------------------------------------------------------------------------------------- */
/* 0 for a shape the entry point refuses. */
size_t oai_visit_slopes_workspace_bytes(long long n_rows, long long n_verts, long long n_subjects, long long n_visits);
int oai_visit_slopes(const float* values_dev, const unsigned char* mask_dev, long long n_rows, long long n_verts, const int* subject_offsets_dev,
                     long long n_subjects, const int* visit_row_dev, const double* visit_time_dev, long long n_visits,
                     const double* reference_time_dev, int min_visits, double min_span, void* workspace_dev, size_t workspace_bytes,
                     double* rate_dev, double* avg_dev, double* fit_ref_dev, double* resid_sd_dev, int* n_dev, unsigned char* out_mask_dev,
                     void* stream);


/* ------------------------------------------------------------------------------------------
 * Normative deviation (csrc/normative.hip, tests/normative_ref.py): where is ONE knee abnormally thin or thick for its age, sex and BMI,
 * and is that more than chance over the whole surface?  A linear model y ~ Z gamma is fitted per vertex on a reference cohort (healthy
 * knees, or the rate maps of non-progressors), and a knee is scored against it vertex by vertex: its residual over the standard error of
 * a NEW observation, which accounts for the covariates, for the uncertainty of the fitted mean (the leverage of the knee's design row)
 * and -- for a knee that belongs to the reference -- for the knee's own share in the fit.  The reference has no such step: the
 * definitions are this library's own, pinned by the numpy restatement and by refits with numpy.linalg.lstsq.  The design Z is float64
 * [n_knees][p], knee-major, 1 <= p <= 6 WITH THE INTERCEPT (if any) COUNTED IN p.  The rules of "Cohort statistics" hold: fp64 without
 * contraction, one accumulator per sum that starts at +0.0, EVERY SUM OVER KNEES IN ASCENDING KNEE INDEX, a missing entry skipped by a
 * select (what lies under a 0 mask byte reaches no sum), no floating-point atomics: bit-reproducible.  Nothing synchronises or reads
 * anything back.  2 <= n_knees <= 2^24, 1 <= n_verts <= 2^31 - 2, at most 2^20 rows per call.  y_dev and mask_dev as in "Cohort
 * statistics"; a null mask: every entry is valid, and the results are THE SAME BITS as with a mask of all ones.
 *
 * oai_normative_fit.  Per vertex v, with m_i the mask and y_i = (double)y[i][v], i = 0 .. n_knees - 1:
 *   n    = sum m_i
 *   A_ac = sum_i (m_i ? z_ia*z_ic : 0.0), c <= a             h_a = sum_i (m_i ? z_ia*y_i : 0.0)
 *   A = L L^T, with the order and the PIVOT RULE of "Cohort regression": pivot s is accepted iff s > 1e-10 * A_aa
 *   L w = h forward and L^T gamma = w backward, as stated there
 *   e_i  = y_i - sum_a z_ia*gamma_a                           (from y_i, s = s - z_ia*gamma_a, a ascending)
 *   rss  = sum_i (m_i ? e_i*e_i : 0.0)
 *   ok   = every pivot accepted && n - p >= 1
 * The values are NOT centred: centre the covariate columns instead.  The MODEL BLOCK, model_dev, front to back, each array starting on
 * the next multiple of 256 bytes, COMPONENT-MAJOR so that a wave's 64 consecutive vertices load contiguously: gamma float64 [p][n_verts],
 * L float64 [p (p + 1) / 2][n_verts] (entry (a, c), c <= a, is component a (a + 1) / 2 + c), rss float64 [n_verts], n int32 [n_verts],
 * ok uint8 [n_verts].  It does not depend on n_knees and stays valid for as long as the caller keeps it; a caller may also fill it from
 * arrays that it stored.  A thread owns one vertex; the sum over knees is not split.
 *
 * oai_normative_score: n_rows knees -> the z tile, float64 [n_rows][n_verts] at the start of workspace_dev, in the layout that
 * oai_graph_clusters and oai_graph_tfce consume (rows = knees).  x_dev float32 [n_rows][n_verts]; x_mask_dev uint8 [n_rows][n_verts] or
 * null (every entry valid); design_rows_dev float64 [n_rows][p], the design row g of each knee, built as the columns of Z were.  Per
 * (row k, vertex v), with x = (double)x[k][v], mx the row's mask byte there, and the per-call flag loo:
 *   e   = x - sum_a g_a*gamma_a                               (from x, s = s - g_a*gamma_a, a ascending)
 *   L u = g forward                                           (u_a = (g_a - sum_{k<a} L_ak*u_k) / L_aa, s = s - L_ak*u_k, k ascending)
 *   lev = sum_a u_a*u_a                                       (from +0.0, a ascending: the leverage g^T (Z^T Z)^-1 g)
 *   loo = 0 (a knee that is NOT in the fit; the prediction-interval t):
 *     dof = n - p;  s2 = rss/dof;  se2 = s2*(1.0 + lev)
 *   loo = 1 (row k is the fit's own row k, x and mask as fitted; the externally studentised residual, identical to scoring the knee
 *            against a fit without it):
 *     den = 1.0 - lev;  dof = n - p - 1;  s2 = (rss - (e*e)/den)/dof;  se2 = s2*den
 *   z   = e / sqrt(se2)
 *   z is valid iff mx && ok && dof >= 1 && s2 > 0 && (loo == 0 || den > 1e-10), otherwise NaN
 * den > 1e-10 is A CONDITION and part of the contract, like the pivot rule: a knee that alone carries a design direction (the only
 * member of a dummy level) has leverage 1 and no leave-one-out score.  diff_dev float64 [n_rows][n_verts], or null: receives e, the
 * deviation in mm, where mx && ok and NaN elsewhere.  There is no float32 output of z.  A thread owns one vertex and eight rows, so that
 * gamma, L, rss, n and ok are loaded once per eight rows; the design rows are wave-uniform.
 *
 * oai_deviation_summary: per row of a z tile (tile_dev float64 [n_rows][n_verts]) at a threshold z0 > 0, over the entries that are not
 * NaN: stats_dev float64 [n_rows][3] = (max |z|, min z, max z) -- 0.0, NaN, NaN for a row without a valid entry; counts_dev int64
 * [n_rows][6] = (n_valid, the vertex of max |z|: THE SMALLEST INDEX AT A TIE, -1 without a valid entry; the vertex count of {z < -z0} and
 * its area; the vertex count of {z > z0} and its area).  Both sets are strict.  An area is the int64 sum of weight_dev int64 [n_verts]
 * over the set (the integer vertex areas in units of 2^-20 mm^2 that "Threshold-free cluster enhancement" takes; null: every weight is
 * 1): an integer sum, so no order needs stating; maxima and minima are exact.
 * ---------------------------------------------------------------------------------------- */
/* All three: 0 for a shape the entry point refuses.  oai_normative_fit_workspace_bytes is the size of the model block. */
size_t oai_normative_fit_workspace_bytes(long long n_verts, int n_columns);
int oai_normative_fit(const float* y_dev, const unsigned char* mask_dev, const double* design_dev, long long n_knees, long long n_verts, int n_columns,
                      void* model_dev, size_t model_bytes, void* stream);
size_t oai_normative_score_workspace_bytes(long long n_rows, long long n_verts);
int oai_normative_score(const void* model_dev, size_t model_bytes, const float* x_dev, const unsigned char* x_mask_dev, const double* design_rows_dev,
                        long long n_rows, long long n_verts, int n_columns, int loo, void* workspace_dev, size_t workspace_bytes, double* diff_dev,
                        void* stream);
size_t oai_deviation_summary_workspace_bytes(long long n_rows, long long n_verts);
int oai_deviation_summary(const double* tile_dev, long long n_rows, long long n_verts, const long long* weight_dev, double z0, void* workspace_dev,
                          size_t workspace_bytes, double* stats_dev, long long* counts_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Bootstrap intervals (csrc/bootstrap.hip, tests/bootstrap_ref.py): how large is an effect, give or take what -- the coefficient of the
 * LAST column of the per-vertex general linear model of "Cohort regression", re-estimated on resamples of the knees, and what a
 * percentile, basic or BCa interval and a simultaneous sup-t band need from the replicates.  BCa (Efron 1987) and the sup-t band (Davison
 * and Hinkley 1997) are as recalled and NOT pinned to any implementation; the reference has no such step, and the definitions are this
 * library's own, pinned by the numpy restatement and, through it, scipy.stats.bootstrap.  The rules of "Cohort statistics" hold: fp64
 * without contraction, no floating-point atomics, one accumulator per sum that starts at +0.0, EVERY SUM OVER KNEES AND OVER REPLICATES IN
 * ASCENDING INDEX: bit-reproducible.  Nothing synchronises or reads anything back.  2 <= n_knees <= 2^24, 1 <= n_verts <= 2^31 - 2, at
 * most 2^20 rows per call.  y_dev and mask_dev as in "Cohort statistics"; design_dev float64 [n_knees][p], knee-major, 1 <= p <= 6.
 *
 * oai_bootstrap_coef: one resample is a row of integer weights on the knees, counts_dev uint16 [R][n_knees]: how often knee i enters
 * row r.  Rows [r0, r1) on the vertex span [v0, v1) -> the tile float64 [r1 - r0][v1 - v0] at the start of workspace_dev.  Per
 * (row r, vertex v), knees i ascending, g_i the design row of knee i and G_iac = g_ia*g_ic (formed once per call, in fp64):
 *   w_i  = m_iv ? (double)c_ri : 0.0          the weight is chosen by a select; a missing entry is never multiplied in: y enters as
 *   u_i  = w_i * (double)y_iv                   m_iv ? (double)y_iv : 0.0.  The product is exact: 24 + 16 bits
 *   h_a  = h_a + g_ia * u_i                   a product THEN an add
 *   M_ac = M_ac + w_i * G_iac, c <= a         a product THEN an add, not an fma: w*G is not exact for w > 1
 *   M = L L^T with the order and the pivot rule of "Cohort regression";  L z = h forward;  theta = z_p / L_pp
 *   theta is NaN when a pivot was not accepted: a resample that lost the rank among the valid knees, a group drawn empty, a vertex
 *   without values.
 * With r0 = 0, n_dev and ok_dev (int32 [n_verts], entries [v0, v1) written; either may be null) receive n_v = sum_i m_iv and ok_v = every
 * pivot of row 0 accepted.  mask_dev null: every entry is valid, M_r = sum_i c_ri*G_i does not depend on the vertex and is formed and
 * factored once per row, in the same order, and the results are THE SAME BITS as with a mask of all ones.  A thread owns one vertex and
 * R rows (R depends on p and on whether there is a mask).
 *
 * oai_bootstrap_moments: per vertex of a tile [n_rows][n_verts] whose row 0 is the observed data, over rows 1 .. n_rows - 1 ascending:
 *   B' = the number of finite entries;  mean* = (sum theta*) / (double)B';  se = sqrt(sum (theta* - mean*)^2 / (double)(B' - 1)), two
 *   passes, centred on the mean of pass 1, NaN for B' < 2;  below = #{theta* < theta^}, equal = #{theta* == theta^} among the finite
 *   entries, theta^ the entry of row 0.  All five outputs [n_verts]: n_finite, below, equal int32; mean, se float64.
 *
 * oai_column_quantiles: exact order statistics per vertex of rows [first_row, n_rows) of a tile, K <= 4 probabilities, either shared
 * (probs_host, K host doubles) or per vertex (probs_dev float64 [K][n_verts]); exactly one of the two is not null.  out_dev float64
 * [K][n_verts], count_dev int32 [n_verts] = n', the entries that are not NaN.  Over those n' entries this is numpy >= 2's
 * method="linear" in float64: vi = (double)(n' - 1) * q;  fl = floor(vi);  gamma = vi - fl;  at or past n' - 1 the last element with
 * gamma = 0;  then numpy's _lerp: a + (b - a)*t for t < 0.5, else b - (b - a)*(1 - t).  n' = 0, a NaN probability or one outside [0, 1]
 * gives NaN.  The order is the total order of the order-preserving 64-bit key map (u with the sign bit set: ~u, otherwise u | 2^63), so
 * -0.0 sorts before +0.0: the value of np.quantile everywhere, and its bits except for the sign of a zero.  ONE PATH FOR EVERY
 * 1 <= n_rows <= 2^20: the tile is transposed to vertex-major keys in the workspace, then an 8-pass radix select per vertex.
 *
 * oai_bootstrap_sup: per row r of a tile, sup_r = max over the vertices of |theta*_rv - theta^_v| / se_v -- a subtract, an abs and a
 * divide -- where theta^_v is finite and se_v > 0, skipping NaN entries by a select; sup_dev float64 [n_rows] is a running maximum that
 * the caller starts at 0.0 and the call raises: sup[r] = max(sup[r], sup_r), so it folds across vertex spans.  A max is exact in any
 * order.
 *
 * oai_jackknife_acceleration: jack_dev float64 [n_knees][v1 - v0] is the tile of oai_bootstrap_coef for the n_knees count rows "all
 * ones except a 0 at knee i"; stratum_dev int32 [n_knees] labels 0 .. n_strata - 1 (a knee with another label is in no stratum).  Per
 * vertex, strata s ascending, over the knees of s valid at v, ascending:
 *   n_s;  mean_s = (sum theta_(i)) / (double)n_s;  U_i = (double)(n_s - 1) * (mean_s - theta_(i));  sum U_i*U_i and sum (U_i*U_i)*U_i
 *   num = num + (sum U^3) / (n_s*n_s*n_s);  den = den + (sum U^2) / (n_s*n_s)         (n_s as a double; an empty stratum is skipped)
 *   a = (num / (den * sqrt(den))) / 6.0       the acceleration scipy.stats.bootstrap uses, the textbook one for a single stratum
 *   a is NaN where den > 0 does not hold or any theta_(i) of a valid knee is NaN.  accel_dev float64 [v1 - v0].
 * ---------------------------------------------------------------------------------------- */
/* Both *_workspace_bytes: 0 for a shape the entry point refuses, a multiple of 256 otherwise. */
size_t oai_bootstrap_coef_workspace_bytes(long long n_rows, long long n_span, long long n_knees, int n_columns);
int oai_bootstrap_coef(const float* y_dev, const unsigned char* mask_dev, const double* design_dev, const unsigned short* counts_dev, long long n_knees,
                       long long n_verts, int n_columns, long long v0, long long v1, long long r0, long long r1, void* workspace_dev,
                       size_t workspace_bytes, int* n_dev, int* ok_dev, void* stream);
int oai_bootstrap_moments(const double* tile_dev, long long n_rows, long long n_verts, int* n_finite_dev, double* mean_dev, double* se_dev,
                          int* below_dev, int* equal_dev, void* stream);
size_t oai_column_quantiles_workspace_bytes(long long n_rows, long long n_verts);
int oai_column_quantiles(const double* tile_dev, long long n_rows, long long n_verts, long long first_row, int n_probs, const double* probs_host,
                         const double* probs_dev, void* workspace_dev, size_t workspace_bytes, double* out_dev, int* count_dev, void* stream);
int oai_bootstrap_sup(const double* tile_dev, long long n_rows, long long n_verts, const double* se_dev, double* sup_dev, void* stream);
int oai_jackknife_acceleration(const double* jack_dev, const unsigned char* mask_dev, const int* stratum_dev, long long n_knees, long long n_verts,
                               long long v0, long long v1, int n_strata, double* accel_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Rank transform (csrc/rank_transform.hip, tests/rank_transform_ref.py): per vertex the midranks of the knees that have a value there,
 * the rank sums of groups of knees, and scores of the ranks -- what Mann-Whitney, Wilcoxon signed-rank, Kruskal-Wallis, Spearman and
 * the rank-based inverse-normal transform start from.  The reference has no such step; the definitions are this library's own, pinned
 * by a restatement through scipy.stats.rankdata and, through it, scipy's own tests.  values_dev float32 [n_knees][n_verts] (knee-major,
 * the cohort's own layout) and mask_dev uint8 [n_knees][n_verts] or null, as in "Cohort statistics".  Nothing synchronises or reads
 * anything back.  1 <= n_knees <= 2^22, so a midrank is exact in float32; 1 <= n_verts <= 2^31 - 2.
 *
 * oai_column_ranks, mode OAI_RANK_PLAIN or OAI_RANK_SIGNED.
 *   Validity.  An entry is valid iff its mask is non-zero (every entry, with a null mask) and its value is not NaN.  In signed mode the
 *     value must also be != 0.0f: scipy's zero_method="wilcox" drops zeros before ranking.
 *   Key.  The key is y in plain mode and fabsf(y) in signed mode.  Comparison is float < and ==, so -0.0 ties +0.0, and +-inf are
 *     ordinary values.
 *   Rank.  For a valid entry i at vertex v, over the valid j at v:
 *     less_i  = #{j: k_j < k_i}
 *     equal_i = #{j: k_j == k_i}                 (i itself included)
 *     twice_rank_i = 2*less_i + equal_i + 1      twice the midrank of scipy.stats.rankdata(method="average")
 *     In signed mode the result is negated where y < 0.
 *   Outputs.  twice_rank_dev int32 [n_knees][n_verts], 0 where the entry is not valid; n_valid_dev int32 [n_verts];
 *     tie_term_dev int64 [n_verts] = sum over valid i of (equal_i^2 - 1), which equals the sum over tie groups of (t^3 - t), the
 *     correction that Kruskal-Wallis and the asymptotic variances use.
 *   Everything is an integer count, so the result does not depend on launch geometry or on the order anything ran in (the one atomic
 *   is a 64-bit integer add).  The form is O(n_knees^2 n_verts) compares: a lane owns a vertex and sixteen of its rows and walks all
 *   rows once per sixteen.
 *
 * oai_rank_sums: labels_host uint8 [n_knees], A HOST ARRAY, the group 0 .. n_groups - 1 of every knee, 1 <= n_groups <= 16; a label
 * >= n_groups is refused before any launch, which is why the labels are not a device array.  n_g_dev int32 [n_groups][n_verts] = the
 * valid entries (twice_rank != 0) of group g; twice_sum_g_dev int64 [n_groups][n_verts] = sum of |twice_rank| over them.  labels_host
 * null: n_groups must be 2, and group 0 is the negative entries and group 1 the positive ones -- 2 W- and 2 W+ of the signed ranks.
 * Integer sums: exact in any order.
 *
 * oai_rank_scores: twice_rank_dev and n_valid_dev as oai_column_ranks wrote them, a kind and a constant c in [0, 1/2] (read by
 * OAI_SCORE_NORMAL alone) -> score_dev float64 [n_knees][n_verts] and mask_dev uint8 [n_knees][n_verts] = (twice_rank != 0); the score
 * of an entry that is not valid is 0.0.
 *   OAI_SCORE_RANK:     0.5 * twice_rank, sign kept.  Exact.
 *   OAI_SCORE_CENTRED:  0.5 * twice_rank - 0.5 * (n_valid + 1).  Exact.
 *   OAI_SCORE_NORMAL:   Phi^-1((r - c) / (n_valid - 2c + 1)) with r = 0.5 * |twice_rank|, the sign of twice_rank re-applied (signed
 *     mode); the probability is formed in float64 as (r - c) / ((n - 2.0*c) + 1.0).  The named constants: Blom 3/8 (the default of
 *     the Python layer), Tukey 1/3, Bliss-Rankit 1/2, van der Waerden 0.  The default is as recalled from PALM's -inormal and is
 *     pinned to no implementation.
 *   Phi^-1 on the device: work on the lower tail, q = min(p, 1 - p); start from x = -sqrt(-2 ln q), or from 2.5 (q - 1/2) when
 *   q > 0.2; four Halley steps on erfc(-x / sqrt 2) / 2 - q: u = (F - q) / phi(x), x <- x - u / (1 + x u / 2); mirror for p > 1/2.  Four
 *   is the smallest count at which the comparison with scipy.special.ndtri no longer improves.  The device erfc, exp and log are not
 *   numpy's: this ONE output is held to a tolerance, not to the bit (tests/test_rank_transform_gpu.py states the measured error and the
 *   gate).
 * ---------------------------------------------------------------------------------------- */
#define OAI_RANK_PLAIN 0
#define OAI_RANK_SIGNED 1
#define OAI_SCORE_RANK 0
#define OAI_SCORE_CENTRED 1
#define OAI_SCORE_NORMAL 2
int oai_column_ranks(const float* values_dev, const unsigned char* mask_dev, long long n_knees, long long n_verts, int mode, int* twice_rank_dev,
                     int* n_valid_dev, long long* tie_term_dev, void* stream);
int oai_rank_sums(const int* twice_rank_dev, const unsigned char* labels_host, long long n_knees, long long n_verts, int n_groups, int* n_g_dev,
                  long long* twice_sum_g_dev, void* stream);
int oai_rank_scores(const int* twice_rank_dev, const int* n_valid_dev, long long n_knees, long long n_verts, int kind, double c, double* score_dev,
                    unsigned char* mask_dev, void* stream);


/* ------------------------------------------------------------------------------------------
 * Cohort PCA (csrc/cohort_pca.hip, tests/cohort_pca_ref.py): the area-weighted, missing-aware principal components of a cohort's
 * thickness maps by way of the N x N Gram matrix of the whitened knees (the snapshot method), and what scoring a knee against the
 * model needs: Hotelling's T2 inside it and the residual Q (squared prediction error) outside it.  The reference has no such step;
 * the definitions are this library's own, pinned by a numpy restatement that is held to np.linalg.svd and sklearn.  The eigen-
 * decomposition itself is N x N and runs on the host (np.linalg.eigh); the three entry points below are what is O(N V) and O(N^2 V).
 * Nothing synchronises or reads anything back.
 *
 * The inputs.
 *   Y: float32 [N][V], knee-major.
 *   M: uint8 mask, may be null.  Validity is as everywhere else: the mask is non-zero and the value is not NaN.
 *   mean: float64 [V].
 *   rw: float64 [V], the root weights, sqrt(area in mm^2).  The host takes the square root with np.sqrt, so the device takes no
 *     square root.
 *
 * Whitening.  a_iv = ((double)Y_iv - mean_v) * rw_v is one subtraction followed by one product.  Where the entry is missing or
 *   rw_v == 0, a_iv is exactly 0.0 by a select, never by a product.  A vertex with no valid knee has a NaN mean and must not leak.
 *
 * Ordered dot.  C_ij = sum over v of a_iv * b_jv.  The order is the contract:
 *   The vertex axis is cut into chunks of 512 consecutive vertices.  The last chunk is short.
 *   Inside a chunk, the terms are added in ascending v into one accumulator that starts at 0.0.  It is a product, then an add, with
 *     no FMA.
 *   The chunk sums are then added in ascending chunk index into one accumulator that starts at 0.0.
 *   The float64 product is commutative, so C of (A, A) is symmetric to the bit.
 *   The vector fp64 MFMA is deliberately not used.  Its internal summation order cannot be restated in numpy.
 *
 * Ordered combine.  R_cv = sum over i of k_ci * a_iv, summed over ascending i into one accumulator, product then add.
 *
 * oai_cohort_whiten writes A = out_dev float64 [n_knees][n_verts] and, where norm2_dev is not null, norm2_i = sum over v of a_iv^2
 *   in the ordered-dot order, float64 [n_knees]: the diagonal of oai_rows_cross(A, A), from which the Q of a new knee is read without
 *   an N' x N' product.  1 <= n_knees <= 2^24 (one knee is scored against a model alone), 1 <= n_verts <= 2^31 - 2.
 * oai_rows_cross writes out_dev float64 [n_a][n_b], C of the rows a_dev [n_a][n_verts] and b_dev [n_b][n_verts];
 *   1 <= n_a, n_b <= 2^20.  With b_dev == a_dev (and n_b == n_a) it computes only the tiles on or above the diagonal and mirrors
 *   them.  Two execution forms of one device body.  Walk: one workgroup per 64 x 64 output tile walks all chunks, no workspace.
 *   Split: a grid of tiles x chunks, each workgroup writes its tile's chunk sum to the workspace and a finish kernel adds the chunk
 *   sums in ascending chunk index.  The split form runs when workspace_dev is not null and ceil(n_a / 64) * ceil(n_b / 64) <= 256;
 *   it needs oai_rows_cross_workspace_bytes(n_a, n_b, n_verts) bytes (0 for shapes it refuses and for tile counts above 256) and a
 *   smaller workspace is refused.  Both forms give the same bits by construction.
 * oai_rows_combine writes out_dev float64 [n_out][n_verts] = R of coef_dev float64 [n_out][n_rows] and rows_dev float64
 *   [n_rows][n_verts]; 1 <= n_out, n_rows <= 2^20.
 * Both product entry points are plain row-matrix primitives on float64 rows and know nothing of thickness.
 *
 * Limits.  Mean imputation: a missing entry contributes 0 after centring; the Python layer reports it through n_missing and
 * n_excluded.  No leave-one-out member scores.  No choice of K and no parallel analysis.  eigh on the host.  Degenerate (equal)
 * eigenvalues leave their modes defined only up to rotation.  No fp64 MFMA path.  No thresholds.
 * ---------------------------------------------------------------------------------------- */
int oai_cohort_whiten(const float* values_dev, const unsigned char* mask_dev, const double* mean_dev, const double* root_weight_dev,
                      long long n_knees, long long n_verts, double* out_dev, double* norm2_dev, void* stream);
size_t oai_rows_cross_workspace_bytes(long long n_a, long long n_b, long long n_verts);
int oai_rows_cross(const double* a_dev, long long n_a, const double* b_dev, long long n_b, long long n_verts, double* out_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);
int oai_rows_combine(const double* coef_dev, const double* rows_dev, long long n_out, long long n_rows, long long n_verts, double* out_dev,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OAI_HIP_H */
