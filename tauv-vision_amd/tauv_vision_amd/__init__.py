"""tauv_vision_amd — MI355X-native (gfx950) drop-in for TAUV-Vision's per-frame CenterNet
detection path: `Centernet(DLABackbone(...), object_config)(img) -> Prediction`, then
`decode` / `decode_keypoints`, with all compute in hand-written HIP kernels
(lib/libtauv_vision_amd.so, C ABI in include/tauv_vision_amd.h)."""
from .config import AngleConfig, ModelConfig, ObjectConfig, ObjectConfigSet, TrainConfig  # noqa: F401
from .centernet import (CenterpointDLA34, Centernet, CenternetDetections, CenternetDetector,  # noqa: F401
                        CenternetPoseDetections, Prediction, get_head_channels, initialize_weights, preprocess)
from .dla import DLABackbone  # noqa: F401
from .decode import (Detection, DeviceAngleDecoder, DeviceDecoder, DeviceKeypointDecoder,  # noqa: F401
                     DevicePoseSolver, KeypointDetection, KeypointRecords, angle_decode, angle_get_bins,
                     angle_ranges, decode, decode_keypoint_poses, decode_keypoints, decode_keypoints_records,
                     decode_oriented, decode_oriented_records, decode_records, depth_decode, heatmap_detect,
                     heatmap_nms, keypoint_detections_from_records, pose_model_points)
from .yolact import (DeviceFrameMasks, FeaturePyramid, FrameMasks, Masknet, PredictionHead,  # noqa: F401
                     Resnet101Backbone, TAB10, Yolact, YolactConfig, YolactDetections, YolactDetector, YolactHead,
                     detection_records, frame_masks, pack_frame_masks, unpack_frame_masks, yolact_head_state_dict)
from .localize import DeviceLocalizer, localize_detections, localize_masks  # noqa: F401
# the module stays `tauv_vision_amd.evaluate` (the reference's scripts are evaluate.py / evaluate_keypoints.py)
from .evaluate import (DeviceEvaluator, EvaluationResult, evaluate_keypoints_precision_recall,  # noqa: F401
                       evaluate_keypoints_precision_recall_curve, evaluate_precision_recall,
                       evaluate_precision_recall_curve)
from .yolact_evaluate import (DeviceYolactEvaluator, YolactEvaluation, average_precision,  # noqa: F401
                              evaluate_average_precision)
# the loss itself is tauv_vision_amd.loss.loss (`from tauv_vision_amd.loss import loss`, as the reference's
# train.py imports it): the package attribute `loss` stays the module
from .loss import (Angle, Losses, PoseSample, angle_in_range, angle_loss, angle_range, depth_loss,  # noqa: F401
                   focal_loss, generate_heatmap, generate_keypoint_heatmap, out_index_for_position)
from .augment import (AugmentParams, DeviceAugmenter, SegmentationSample, augment_pose_batch,  # noqa: F401
                      augment_segmentation_batch, identity_params, params_from_matrices, sample_centernet_params,
                      sample_yolact_params, transform_boxes, transform_points)

__version__ = "0.1.0"
