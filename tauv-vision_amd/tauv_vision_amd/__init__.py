"""tauv_vision_amd — MI355X-native (gfx950) drop-in for TAUV-Vision's per-frame CenterNet
detection path: `Centernet(DLABackbone(...), object_config)(img) -> Prediction`, then
`decode` / `decode_keypoints`, with all compute in hand-written HIP kernels
(lib/libtauv_vision_amd.so, C ABI in include/tauv_vision_amd.h)."""
from .config import AngleConfig, ModelConfig, ObjectConfig, ObjectConfigSet, TrainConfig  # noqa: F401
from .centernet import (CenterpointDLA34, Centernet, CenternetDetections, CenternetDetector, Prediction,  # noqa: F401
                        get_head_channels, initialize_weights, preprocess)
from .dla import DLABackbone  # noqa: F401
from .decode import (Detection, DeviceKeypointDecoder, KeypointDetection, KeypointRecords, angle_decode,  # noqa: F401
                     angle_get_bins, decode, decode_keypoints, decode_keypoints_records, decode_records, depth_decode,
                     heatmap_detect, heatmap_nms, keypoint_detections_from_records)
from .yolact import (FeaturePyramid, Masknet, PredictionHead, Resnet101Backbone, Yolact, YolactConfig,  # noqa: F401
                     YolactDetections, YolactDetector, YolactHead, detection_records, yolact_head_state_dict)
from .localize import DeviceLocalizer, localize_detections, localize_masks  # noqa: F401

__version__ = "0.1.0"
