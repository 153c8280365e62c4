"""image_segmentation_amd -- MI355X-native segmentation forward/backward hot path
(drop-in for the reference's unet/unet.py, clip/clipunet.py decoder, autoencoder/autoencoder.py family,
utils/weighted_loss.py losses and the utils/training.py loops).  Requires the in-tree HIP library (python -m image_segmentation_amd.build)."""
from .ops import set_compute_dtype, get_compute_dtype      # noqa: F401
from .unet import unet, DoubleConvReLU, Down, Up             # noqa: F401
from .losses import (CrossEntropyLoss, MSELoss, WeightedMemoryEfficientDiceLoss, WeightedDiceCELoss,     # noqa: F401
                     WeightedMemoryEfficientDiceLossPrompt, WeightedDiceNLLLoss, HardPixelLoss, FocalLoss,
                     OhemCrossEntropyLoss, LovaszSoftmaxLoss, LovaszCELoss)
from .clipunet import ClipUNet, UNetDecoder, DecoderBlock, ClipViTEncoder                   # noqa: F401
from .autoencoder import SegmentationAutoencoder, ReconstructionAutoencoder               # noqa: F401
from .prompt import PromptModel                                                            # noqa: F401
from .inference import Segmenter, Prediction, predict, load_checkpoint, COLOR_MAP, CLASS_NAMES   # noqa: F401
from .prompts import PromptSampler, PromptBatch, PromptBatches, TRIMAP_TO_PROMPT, heat_tables, point_heatmap   # noqa: F401
from .augment import (Augmenter, AugPlan, AugmentedBatches, merge_pairs, class_weights, convert_rgb_label_to_classes,   # noqa: F401
                      cubic_table, contrast_lut, laplace_table, rotation_plan, merge_plan, ALL_OPS, TARGET_REMAP)
from .robustness import (PERTURBATIONS, DEFAULT_LEVELS, PerturbPlan, gauss_table, value_lut, perturb_plan, perturb,      # noqa: F401
                         robustness_sweep, cell_seed, image_seed)
from .tta import TTA, view_table, view_order, VIEW_DESC                                                      # noqa: F401
from .tiles import Tiles, tile_axis, tile_plan                                                                # noqa: F401
from .components import components, Components, Clean, mask_finish                                          # noqa: F401
from .vectors import vectorize, Vectors, default_capacities                                                 # noqa: F401
from .raster import (Shape, rasterize, rasterize_batch, shapes_from_coco, shapes_from_vectors, rle_to_string,   # noqa: F401
                     rle_from_string, raster_plan)
from .morph import (erode, dilate, open_mask, close_mask, label_band, boundary_distance, fill_holes, Filled,       # noqa: F401
                    MorphStep)
from .mix import Mixer, MixPlan, MixedBatches                                                                      # noqa: F401
from .panoptic import match_objects, ObjectMatch, PanopticQuality, object_quality, quality_from_stats              # noqa: F401
from .boundary import boundary_stats, BoundaryStats, BoundaryQuality, boundary_quality, quality_from_boundary_stats  # noqa: F401
from .superpixels import superpixels, snap_mask, Superpixels, Snapped, Snap                                         # noqa: F401
from .calibration import (Reliability, reliability, TemperatureFit, fit_temperature, refine_temperature,            # noqa: F401
                          default_temperatures, inverse_temperatures, fit_from_counts)
from .distill import Teacher, TeacherViews, DistillLoss, teacher_table, TEACHER_DESC                                 # noqa: F401
from .training import train_loop, eval_loop, train_loop_distill                                                      # noqa: F401
from .optim import AdamW                                                                                            # noqa: F401
