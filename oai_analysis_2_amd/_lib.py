"""ctypes binding of liboai_hip.so (include/oai_hip.h).  Fails loudly: there is no fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OAI_LIB_PATH") or os.path.join(HERE, "liboai_hip.so")   # override: diagnostic builds only


class OaiError(RuntimeError):
    pass


class Affine(C.Structure):
    _fields_ = [("A", C.c_double * 9), ("b", C.c_double * 3)]


class LayerParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("cin", C.c_int), ("cout", C.c_int),
                ("weight", C.c_void_p), ("bias", C.c_void_p),
                ("bn_gamma", C.c_void_p), ("bn_beta", C.c_void_p), ("bn_mean", C.c_void_p), ("bn_var", C.c_void_p)]


class IconUnetParams(C.Structure):
    _fields_ = [("down_w", C.c_void_p * 5), ("down_b", C.c_void_p * 5),
                ("up_w", C.c_void_p * 5), ("up_b", C.c_void_p * 5),
                ("bn_gamma", C.c_void_p * 5), ("bn_beta", C.c_void_p * 5),
                ("bn_mean", C.c_void_p * 5), ("bn_var", C.c_void_p * 5),
                ("last_w", C.c_void_p), ("last_b", C.c_void_p)]


class IconNode(C.Structure):              # == struct oai_icon_node
    _fields_ = [("kind", C.c_int), ("a", C.c_int), ("b", C.c_int)]


# name -> (restype, argtypes); every symbol declared in include/oai_hip.h
_I, _P, _F, _Z, _D = C.c_int, C.c_void_p, C.c_float, C.c_size_t, C.c_double
_I3 = C.POINTER(C.c_int)
SIGNATURES = {
    "oai_version": (_I, []),
    "oai_last_error": (C.c_char_p, []),
    "oai_device_info": (_I, [C.c_char_p, _I]),
    "oai_grid_sample3d": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P]),
    "oai_compose": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P]),
    "oai_avgpool2_3d": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "oai_resize_trilinear": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "oai_phi_to_itk_displacement": (_I, [_P, _I, _I, _I, _P, _P]),
    "oai_resample_through_disp": (_I, [_P, _I, _I, _I, _P, _I, _I, _I, C.POINTER(Affine), C.POINTER(Affine),
                                       _P, _I, _I, _I, _P]),
    "oai_warp_chain": (_I, [_P, _I, _I, _I, _I, C.POINTER(_P), C.POINTER(_I), _P, _I, _I, _I, _P, _P]),
    "oai_resample_maps_through_phi": (_I, [_P, _I, _I, _I, _I, _P, _I, _I, _I, C.POINTER(Affine), C.POINTER(Affine),
                                           _P, _I, _I, _I, _P]),
    "oai_unet_tile_costs": (_I, [_P, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), _I]),
    "oai_unet_cover_stats": (_I, [_I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, C.POINTER(C.c_double), C.POINTER(C.c_int), _I]),
    "oai_unet_block_list": (_I, [_I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _I, _I, C.POINTER(C.c_uint), _I,
                                 C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "oai_mc_table": (_I, [_P]),
    "oai_mc_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_mc_count": (_I, [_P, _I, _I, _I, _F, _P, _Z, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _P]),
    "oai_mc_emit": (_I, [_P, _I, _I, _I, _F, C.POINTER(C.c_float), _P, _P, _P, _P]),
    "oai_mesh_smooth": (_I, [_P, C.c_longlong, _P, _P, _I, _F, _P, _P, _P]),
    "oai_mesh_point_distance": (_I, [_P, C.c_longlong, _P, _P, C.c_longlong, _P, _P]),
    "oai_mesh_grid_workspace_bytes": (_Z, [C.POINTER(C.c_int), C.c_longlong]),
    "oai_mesh_point_distance_grid": (_I, [_P, C.c_longlong, _P, _P, C.c_longlong, C.POINTER(C.c_float), _F, C.POINTER(C.c_int), _P, _Z, _P, _P]),
    "oai_map_attributes": (_I, [_P, C.c_longlong, _P, _I, _P, C.c_longlong, _D, _P, _P]),
    "oai_point_grid_workspace_bytes": (_Z, [C.POINTER(C.c_int), C.c_longlong]),
    "oai_map_attributes_grid": (_I, [_P, C.c_longlong, _P, _I, _P, C.c_longlong, _D, C.POINTER(_D), _D, C.POINTER(C.c_int), _P, _Z, _P, _P]),
    "oai_point_footprint": (_I, [_P, C.c_longlong, _P, C.c_longlong, _D, _P, _P, _P, _P]),
    "oai_point_footprint_grid": (_I, [_P, C.c_longlong, _P, C.c_longlong, _D, C.POINTER(_D), _D, C.POINTER(C.c_int), _P, _Z, _P, _P, _P, _P]),
    "oai_thickness_map_workspace_bytes": (_Z, [C.c_longlong]),
    "oai_fit_circle": (_I, [_P, C.c_longlong, _I, _I, _P, _Z, C.POINTER(_D), C.POINTER(_D), C.POINTER(_I), _P]),
    "oai_project_circle": (_I, [_P, C.c_longlong, _I, _I, C.POINTER(_D), _P, _P, _P]),
    "oai_project_plateaus": (_I, [_P, _P, C.c_longlong, _P, _Z, _P, _P, _P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _P]),
    "oai_thickness_image_workspace_bytes": (_Z, [C.c_longlong, _I, _I]),
    "oai_thickness_image_build": (_I, [_P, C.c_longlong, _P, C.c_longlong, _P, C.POINTER(_D), C.POINTER(_D), _I, _I, _P, _Z, _P, _P, _P,
                                       C.POINTER(C.c_longlong), _P]),
    "oai_thickness_image_apply": (_I, [_P, _P, _P, _I, _I, _P, C.c_longlong, _I, _P, _P]),
    "oai_mesh_split_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, _I, _I]),
    "oai_mesh_split_features": (_I, [_P, C.c_longlong, _P, C.c_longlong, _I, _P, _Z, _P, _P, C.POINTER(C.c_longlong), _P]),
    "oai_mesh_split_kmeans": (_I, [C.c_longlong, _I, _P, _Z, _P, _I, _I, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(_D), _P,
                                   C.POINTER(_I), _P]),
    "oai_mesh_submesh_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_mesh_submesh": (_I, [_P, C.c_longlong, _P, C.c_longlong, _P, _I, _P, _Z, _P, _P, _P, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _P]),
    "oai_mesh_components_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_mesh_components": (_I, [_P, C.c_longlong, C.c_longlong, _P, _Z, _P, C.POINTER(_I), _P]),
    "oai_mesh_keep_large_regions_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_mesh_keep_large_regions": (_I, [_P, C.c_longlong, _P, C.c_longlong, C.c_longlong, _P, _Z, _P, _P, C.POINTER(C.c_longlong),
                                         C.POINTER(C.c_longlong), _P]),
    "oai_mesh_adjacency_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_mesh_adjacency": (_I, [_P, C.c_longlong, C.c_longlong, _P, _Z, _P, _P, C.POINTER(C.c_longlong), _P]),
    "oai_mesh_grid_params_workspace_bytes": (_Z, []),
    "oai_mesh_grid_params": (_I, [_P, C.c_longlong, _P, C.c_longlong, _P, _Z, _P, _P]),
    "oai_cuberille_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_cuberille_count": (_I, [_P, _I, _I, _I, _F, _P, _Z, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), _P]),
    "oai_cuberille_emit": (_I, [_P, _I, _I, _I, _F, C.POINTER(_D), _I, _I, _I, _D, _D, _D, _I, _I, _P, _Z, C.c_longlong, C.c_longlong,
                                _P, _P, _P, _P]),
    "oai_transform_points_through_phi": (_I, [_P, C.c_longlong, _P, _I, _I, _I, C.POINTER(Affine), C.POINTER(Affine), _P, _P, _P]),
    "oai_phi_jacobian_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_phi_jacobian": (_I, [_P, _I, _I, _I, _P, _P, _Z, _P, _P]),
    "oai_inverse_points_through_phi": (_I, [_P, C.c_longlong, _P, _I, _I, _I, C.POINTER(Affine), C.POINTER(Affine), _I, _D, _P, _P, _P]),
    "oai_invert_phi_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_invert_phi": (_I, [_P, _I, _I, _I, _I, _D, _P, _P, _P, _Z, _P, _P]),
    "oai_mask_overlap_workspace_bytes": (_Z, [C.c_longlong]),
    "oai_mask_overlap": (_I, [_P, _P, C.c_longlong, _F, _P, _Z, _P, _P]),
    "oai_mask_surface": (_I, [_P, _I, _I, _I, _F, _I, _P, _P]),
    "oai_edt_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_edt": (_I, [_P, _I, _I, _I, C.POINTER(_D), _F, _I, _P, _P, _P, _Z, _P, _P]),
    "oai_surface_distance_workspace_bytes": (_Z, [C.c_longlong]),
    "oai_surface_distance": (_I, [_P, _P, _P, _P, C.c_longlong, C.POINTER(_F), _I, _P, _Z, _P, _P]),
    "oai_image_moments_workspace_bytes": (_Z, [C.c_longlong]),
    "oai_image_moments": (_I, [_P, _P, C.c_longlong, _P, _P, _Z, _P, _P]),
    "oai_joint_histogram": (_I, [_P, _P, C.c_longlong, C.POINTER(_F), C.POINTER(_F), _I, _P, _P, _P]),
    "oai_histogram_entropies": (_I, [_P, _I, _P, _P]),
    "oai_lncc_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_lncc": (_I, [_P, _P, _I, _I, _I, C.POINTER(_D), _I, _D, _P, _P, _P, _Z, _P, _P]),
    "oai_label_components_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_label_components": (_I, [_P, _P, _I, _I, _I, _F, _I, _I, C.c_longlong, _P, _P, _P, _Z, _P, _P]),
    "oai_component_sizes": (_I, [_P, C.c_longlong, C.c_longlong, _P, _P]),
    "oai_local_thickness_workspace_bytes": (_Z, [_I, _I, _I]),
    "oai_local_thickness": (_I, [_P, _I, _I, _I, C.POINTER(_D), C.c_longlong, _P, _P, _P, _Z, _P, _P]),
    "oai_masked_stats_workspace_bytes": (_Z, [C.c_longlong]),
    "oai_masked_stats": (_I, [_P, _P, C.c_longlong, C.POINTER(_F), _I, _P, _Z, _P, _P]),
    "oai_mesh_areas_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_mesh_areas": (_I, [_P, C.c_longlong, _P, C.c_longlong, _P, _Z, _P, _P, _P]),
    "oai_region_stats_workspace_bytes": (_Z, [C.c_longlong, _I]),
    "oai_region_stats": (_I, [_P, _P, _P, _P, C.c_longlong, _I, _P, _Z, _P, _P]),
    "oai_mesh_topology_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_mesh_topology": (_I, [_P, C.c_longlong, C.c_longlong, _P, _P, _Z, _P, _P, _P]),
    "oai_mesh_geometry_workspace_bytes": (_Z, [C.c_longlong]),
    "oai_mesh_geometry": (_I, [_P, C.c_longlong, _P, C.c_longlong, _P, C.POINTER(_D), _D, _P, _Z, _P, _P]),
    "oai_mesh_self_intersections_workspace_bytes": (_Z, [C.c_longlong, C.POINTER(C.c_int), C.c_longlong]),
    "oai_mesh_self_intersections": (_I, [_P, C.c_longlong, _P, C.c_longlong, C.POINTER(_D), _D, C.POINTER(C.c_int), C.c_longlong, _P, _Z, _P, _P, _P]),
    "oai_group_prepare_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_group_prepare": (_I, [_P, _P, C.c_longlong, C.c_longlong, _I, _P, _Z, _P]),
    "oai_permutation_t_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_permutation_t": (_I, [_P, _Z, _P, _P, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _I, _P, _Z, _P]),
    "oai_permutation_reduce_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_permutation_reduce": (_I, [_P, C.c_longlong, C.c_longlong, C.c_longlong, _P, _Z, _P, _P, _P, _P]),
    "oai_graph_clusters_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_graph_clusters": (_I, [_P, C.c_longlong, C.c_longlong, _P, _P, C.c_longlong, _D, _P, _Z, _P, _P, _P, _P]),
    "oai_regression_prepare_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_regression_prepare": (_I, [_P, _P, _P, C.c_longlong, C.c_longlong, _I, _I, _P, _Z, _P]),
    "oai_regression_t_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, _I]),
    "oai_regression_t": (_I, [_P, _Z, _P, _P, _P, C.c_longlong, C.c_longlong, _I, C.c_longlong, C.c_longlong, _P, _Z, _P, _P]),
    "oai_regression_f_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, _I]),
    "oai_regression_f": (_I, [_P, _Z, _P, _P, _P, C.c_longlong, C.c_longlong, _I, _I, C.c_longlong, C.c_longlong, _P, _Z, _P, _P]),
    "oai_regression_vx_prepare_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, _I]),
    "oai_regression_vx_prepare": (_I, [_P, _P, _P, _P, _P, C.c_longlong, C.c_longlong, _I, _I, _I, _I, _P, _Z, _P]),
    "oai_regression_vx_t_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, _I, _I]),
    "oai_regression_vx_t": (_I, [_P, _Z, _P, _P, C.c_longlong, C.c_longlong, _I, _I, _I, C.c_longlong, C.c_longlong, _P, _Z, _P, _P]),
    "oai_regression_vx_f_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, _I, _I]),
    "oai_regression_vx_f": (_I, [_P, _Z, _P, _P, C.c_longlong, C.c_longlong, _I, _I, _I, _I, C.c_longlong, C.c_longlong, _P, _Z, _P, _P]),
    "oai_cluster_prepare_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, _I]),
    "oai_cluster_prepare": (_I, [_P, _P, _P, C.c_longlong, C.c_longlong, C.c_longlong, _I, _P, _Z, _P]),
    "oai_cluster_t_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_cluster_t": (_I, [_P, _Z, _P, C.c_longlong, C.c_longlong, C.c_longlong, _I, C.c_longlong, C.c_longlong, _P, _Z, _P, _P, _P]),
    "oai_graph_tfce_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_graph_tfce": (_I, [_P, C.c_longlong, C.c_longlong, _P, _P, C.c_longlong, _P, _D, _D, _I, _I, _I, _P, _Z, _P, _P, _P]),
    "oai_graph_smooth_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_graph_smooth": (_I, [_P, _P, C.c_longlong, C.c_longlong, _P, _P, C.c_longlong, _P, _P, _I, _I, _P, _Z, _P, _P, _P]),
    "oai_visit_slopes_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong]),
    "oai_visit_slopes": (_I, [_P, _P, C.c_longlong, C.c_longlong, _P, C.c_longlong, _P, _P, C.c_longlong, _P, _I, _D, _P, _Z,
                              _P, _P, _P, _P, _P, _P, _P]),
    "oai_normative_fit_workspace_bytes": (_Z, [C.c_longlong, _I]),
    "oai_normative_fit": (_I, [_P, _P, _P, C.c_longlong, C.c_longlong, _I, _P, _Z, _P]),
    "oai_normative_score_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_normative_score": (_I, [_P, _Z, _P, _P, _P, C.c_longlong, C.c_longlong, _I, _I, _P, _Z, _P, _P]),
    "oai_deviation_summary_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_deviation_summary": (_I, [_P, C.c_longlong, C.c_longlong, _P, _D, _P, _Z, _P, _P, _P]),
    "oai_bootstrap_coef_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong, _I]),
    "oai_bootstrap_coef": (_I, [_P, _P, _P, _P, C.c_longlong, C.c_longlong, _I, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _P, _Z,
                                _P, _P, _P]),
    "oai_bootstrap_moments": (_I, [_P, C.c_longlong, C.c_longlong, _P, _P, _P, _P, _P, _P]),
    "oai_column_quantiles_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong]),
    "oai_column_quantiles": (_I, [_P, C.c_longlong, C.c_longlong, C.c_longlong, _I, C.POINTER(_D), _P, _P, _Z, _P, _P, _P]),
    "oai_bootstrap_sup": (_I, [_P, C.c_longlong, C.c_longlong, _P, _P, _P]),
    "oai_jackknife_acceleration": (_I, [_P, _P, _P, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, _I, _P, _P]),
    "oai_column_ranks": (_I, [_P, _P, C.c_longlong, C.c_longlong, _I, _P, _P, _P, _P]),
    "oai_rank_sums": (_I, [_P, _P, C.c_longlong, C.c_longlong, _I, _P, _P, _P]),
    "oai_rank_scores": (_I, [_P, _P, C.c_longlong, C.c_longlong, _I, _D, _P, _P, _P]),
    "oai_cohort_whiten": (_I, [_P, _P, _P, _P, C.c_longlong, C.c_longlong, _P, _P, _P]),
    "oai_rows_cross_workspace_bytes": (_Z, [C.c_longlong, C.c_longlong, C.c_longlong]),
    "oai_rows_cross": (_I, [_P, C.c_longlong, _P, C.c_longlong, C.c_longlong, _P, _P, _Z, _P]),
    "oai_rows_combine": (_I, [_P, _P, C.c_longlong, C.c_longlong, C.c_longlong, _P, _P]),
    "oai_image_normalize_workspace_bytes": (_Z, []),
    "oai_image_normalize": (_I, [_P, _Z, _F, _F, _F, _F, _P, _P, _P, _Z, _P]),
    "oai_partition_tiles": (_I, [_P, _I, _I, _I, _I3, _I3, _I, _I, _P, _P]),
    "oai_assemble_vote": (_I, [_P, _I, _I, _I, _I, _I3, _I3, _P, _P]),
    "oai_unet_create": (_I, [C.POINTER(LayerParams), _F, C.POINTER(_P)]),
    "oai_unet_destroy": (None, [_P]),
    "oai_unet_set_precision": (_I, [_P, _I]),
    "oai_unet_range_flag": (_I, [_P, _I, C.POINTER(_I), _P]),
    "oai_unet_range_flag_snapshot": (_I, [_P, _P, _P]),
    "oai_unet_range_state_snapshot": (_I, [_P, _P, _P]),
    "oai_unet_range_flag_from_state": (_I, [_P, _P, _P]),
    "oai_unet_census": (_I, [_P, C.POINTER(_F), _I, _P]),
    "oai_unet_calibrate_step": (_I, [_P, _P, C.POINTER(_I)]),
    "oai_unet_get_act_exponents": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "oai_unet_set_act_exponents": (_I, [_P, C.POINTER(_I)]),
    "oai_unet_set_option": (_I, [_P, C.c_char_p, _I]),
    "oai_unet_workspace_bytes": (_Z, [_P, _I, _I, _I, _I]),
    "oai_segment_workspace_bytes": (_Z, [_P, _I, _I, _I, _I3, _I3, _I]),
    "oai_unet_forward_tiles": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _Z, _P]),
    "oai_segment_tiles": (_I, [_P, _P, _I, _I, _I, _I3, _I3, _I3, _I, _I, _I, _P, _I, _P, _Z, _P]),
    "oai_unet_volume_flops": (_D, [_P, _I, _I, _I, _I3, _I3, _I3, _I, _I]),
    "oai_warp_set_option": (_I, [C.c_char_p, _I]),
    "oai_stitch_blocks": (_I, [_P, _I, _I, _I, _I, _I3, _I3, _I3, _P, _P]),
    "oai_stitch_blocks_ranged": (_I, [_P, _I, _I, _I, _I, _I3, _I3, _I3, _P, _I, _I, _P, _P]),
    "oai_unet_tile_flops": (_D, [_P, _I, _I, _I, _I3, _I]),
    "oai_unet_tile_flops_conv3": (_D, [_P, _I, _I, _I, _I3, _I]),
    "oai_unet_profile": (_I, [_P, _I]),
    "oai_unet_profile_read": (_I, [_P, C.POINTER(_D), C.POINTER(C.c_longlong)]),
    "oai_icon_create": (_I, [C.POINTER(IconUnetParams), _I, C.POINTER(IconNode), _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "oai_icon_describe": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "oai_icon_destroy": (None, [_P]),
    "oai_icon_workspace_bytes": (_Z, [_P]),
    "oai_icon_forward": (_I, [_P, _P, _P, _P, _P, _Z, _P]),
    "oai_icon_set_graph": (_I, [_P, _I]),
    "oai_icon_set_option": (_I, [_P, C.c_char_p, _I]),
    "oai_icon_graph_info": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "oai_icon_unet_forward": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _Z, _P]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load liboai_hip.so and bind every declared symbol; raise if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64; import it first so that liboai_hip.so binds to the SAME HIP
    # runtime instance (two runtimes in one process do not share devices, streams or allocations).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise OaiError(f"{LIB_PATH} is missing: build it with `python -m oai_analysis_2_amd.build` "
                       "(there is no CPU fallback in this package)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise OaiError(f"liboai_hip.so does not export {name}")
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().oai_last_error()
        raise OaiError(f"{what or 'liboai_hip'} failed ({status}): {msg.decode() if msg else '?'}")


STREAM = object()          # among call()'s arguments: "the current stream of ``device``", wherever the entry point takes its stream


def call(name: str, *args, device=None) -> None:
    """``load().<name>(*args)`` under the calling convention every entry point of the C ABI shares, spelled here and nowhere else:
    the library launches (and a create call allocates) on the current HIP device, so ``device`` is made current around the call; every
    ``STREAM`` among ``args`` becomes that device's current stream; a non-zero status raises OaiError under the symbol's name with
    ``oai_last_error()``.  ``device`` None: a host-only entry point, which touches no GPU and takes no stream."""
    if name not in SIGNATURES:
        raise OaiError(f"{name} is not an entry point of liboai_hip.so (include/oai_hip.h declares none of that name)")
    if device is None:
        if any(a is STREAM for a in args):
            raise ValueError(f"{name}: STREAM stands for the current stream of a device, and no device was given")
        check(getattr(load(), name)(*args), name)
        return
    import torch
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        check(getattr(load(), name)(*[stream if a is STREAM else a for a in args]), name)


def workspace(family: str, device, *size_args, pad: bool = False):
    """The uint8 device buffer that lib.<family>_workspace_bytes(*size_args) asks for.  The library answers 0 for sizes it refuses.
    ``pad``: then one byte all the same, so that the entry point's own argument check names the fault instead of its null-pointer
    check (components and the circle fit, whose callers may pass an empty mesh)."""
    import torch
    n = int(getattr(load(), family + "_workspace_bytes")(*size_args))
    return torch.empty(max(n, 1) if pad else n, dtype=torch.uint8, device=device)


def int3(v):
    return (C.c_int * 3)(int(v[0]), int(v[1]), int(v[2]))
