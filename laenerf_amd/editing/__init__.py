from .style_encoder import LAENeRF, palette_recompose  # noqa: F401
from .editgrid import EditGrid  # noqa: F401
from .mask_lift import lift_masks, mask_iou, mask_lift_numpy, mask_lift_pack, mask_lift_pack_numpy, selection_masks  # noqa: F401
from .edit_dataset import extract_view, extract_views, select_edit_pixels  # noqa: F401
from .recolor import RecolorView, compose_numpy, recolor_views, render_recolored  # noqa: F401
from .style_trainer import EditSet, StyleTrainer, image_terms_on, jitter_numpy  # noqa: F401
from .distill import DistillSet, compose_distill_numpy, distill_images, distill_nerf, distill_steps, error_map_seed_numpy  # noqa: F401
from .style_network import StyleNetwork, load_style_image, load_vgg19_features  # noqa: F401
from .nnfm import nnfm_loss, nnfm_match, nnfm_numpy, nnfm_pack, nnfm_workspace_bytes  # noqa: F401
from .palette_reference import (palet_reg_numpy, palette_backward_numpy, palette_forward_numpy, palette_recompose_bits,  # noqa: F401
                                style_loss_numpy)
from .ray_registration import (RefCloud, extract_ref_cloud, extract_ref_template, ray_registration_numpy, register_rays,  # noqa: F401
                               register_views)
from .semantic_encoder import SemanticEncoder, build_ref_supervision, load_vgg16_features, vgg16_features  # noqa: F401
from .ref_stage import (RefEditSet, RefStyleTrainer, pack_ref_arrays, ref_phase, ref_stage_numpy, ref_terms,  # noqa: F401
                        reference_ref_step, reference_ref_terms)
from .ref_distill import build_ref_distill_data, distill_ref_npr, pack_ref_rows, ref_distill_numpy  # noqa: F401
from .region_transform import (RegionTransform, bake_region_transform, region_occupancy, region_occupancy_numpy, region_warp,  # noqa: F401
                               region_warp_numpy, render_transformed, seed_occupancy, transform_views)
from .scene_insert import (SceneInsert, bake_insert, insert_blend, insert_blend_numpy, insert_occupancy, insert_occupancy_numpy,  # noqa: F401
                           insert_route, insert_route_numpy, insert_views, render_inserted)
