"""The reference's data/ surface without pycocotools and cv2: COCO keypoint annotations in, raw images + keypoints + device-built
mask_miss out (csrc/coco_mask.hip)."""
from .annotations import MaskTables, load_annotations, mask_tables, normalize_annotations, rle_counts
from .dataset import CocoKeypoints, ImageList, collate_raw, raw_batches, read_rgb
from .masks import DeviceMasks, device_masks

__all__ = ['CocoKeypoints', 'DeviceMasks', 'ImageList', 'MaskTables', 'collate_raw', 'device_masks', 'load_annotations', 'mask_tables',
           'normalize_annotations', 'raw_batches', 'read_rgb', 'rle_counts']
