"""Device-side input transforms (reference package `transforms/`, the evaluate.py chain evaluate.py:157-168).

CenterPadNormalize: CenterPad + ToTensor + Normalize as one HIP pass over an already rescaled uint8 image.
EvalPreprocess: the whole chain incl. RescaleLongAbsolute (cv2.resize INTER_CUBIC restated from OpenCV's published 8-bit
algorithm; pinned to the CPU restatement in oracle/, parity with cv2 itself unpinned: cv2 is not available offline), one
kernel per image writing straight into the fp32 batch tensor, host images staged through pinned double buffers; plus the
meta bookkeeping `annotations_inverse` needs.
DeviceAugment: the training side -- WarpAffineTransforms' random flip / rotate / scale / stretch / translate matrix drawn on the host as
the reference draws it, the warp of images and mask_miss, ToTensor + Normalize and the keypoint transform as HIP launches per batch;
with PhotoParams also the reference's RandomApply steps behind the warp: ColorTint, Gray, JpegCompression, AnnotationJitter."""
from .affine import (AugParams, DeviceAugment, FixedAugParams, WarpAffineTransforms, affine_matrix, inverse_rows,  # noqa: F401
                     roi_center)
from .photometric import (AnnotationJitter, ColorTint, Gray, JpegCompression, PhotoParams, RandomApply, draw_photo,  # noqa: F401
                          photo_table)
from .pad import CenterPadNormalize, center_pad_ltrb  # noqa: F401
from .scale import EvalPreprocess, initial_meta, multi_scale_sizes, rescale_meta, rescale_size, resize_cubic  # noqa: F401
