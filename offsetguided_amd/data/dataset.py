"""CocoKeypoints / ImageList (data/dataset.py:14-226) without pycocotools and cv2: the annotation file is read by
annotations.load_annotations, the images by PIL, and mask_miss is not drawn per image on the host but for a whole batch on the device
(collate_raw's tables -> masks.device_masks)."""
import os
import random

import numpy as np

from .annotations import load_annotations, mask_tables, normalize_annotations


def read_rgb(path):
    """(h, w, 3) uint8 RGB, decoded by PIL (the reference: cv2.imread + BGR2RGB)."""
    from PIL import Image
    if not os.path.exists(path):
        raise IOError("image with current path dose not exist: %s" % path)
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'), np.uint8)


class CocoKeypoints:
    """MSCOCO keypoint dataset with the reference's arguments and id filtering: the images with person annotations, in the order of
    the file's `images` list, by default only those with at least one labelled keypoint (filter_for_keypoint_annotations); all_persons
    keeps every image with a person annotation, all_images every image; n_images truncates; shuffle shuffles in place.
    dataset[i] -> (image (h, w, 3) uint8 RGB, record, meta): record = the image's load_annotations record (keypoints, bbox, area,
    iscrowd, num_keypoints, segmentation, height, width), meta = the reference's meta_init.  preprocess(image, record, None, None) ->
    (image, record, meta, _) and target_transforms [t(record, meta, None)] are applied when given.  strict_crowd: an image with more
    than one crowd annotation raises, as the reference's mask_mask does (the device rasteriser gives every crowd its own term)."""

    def __init__(self, img_dir, annFile, *, preprocess=None, target_transforms=None, n_images=None, all_images=False, all_persons=False,
                 shuffle=False, strict_crowd=False):
        self.img_dir = img_dir
        self.annotations = load_annotations(annFile)
        if all_images:
            self.ids = list(self.annotations)
        else:
            self.ids = [image_id for image_id, rec in self.annotations.items() if len(rec['area'])]
            if not all_persons:
                self.filter_for_keypoint_annotations()
        if n_images:
            self.ids = self.ids[:n_images]
        if shuffle:
            random.shuffle(self.ids)
        self.preprocess, self.target_transforms, self.strict_crowd = preprocess, target_transforms, strict_crowd

    def filter_for_keypoint_annotations(self):
        self.ids = [image_id for image_id in self.ids if (self.annotations[image_id]['keypoints'][:, :, 2] > 0.0).any()]

    def __getitem__(self, index):
        image_id = self.ids[index]
        record = self.annotations[image_id]
        if self.strict_crowd and int((record['iscrowd'] == 1).sum()) > 1:
            raise Exception("crowd segments > 1")
        image_path = os.path.join(self.img_dir, record['file_name'])
        image = read_rgb(image_path)
        meta = {'dataset_index': index, 'image_id': image_id, 'file_name': record['file_name'], 'image_path': image_path}
        if 'flickr_url' in record['image']:
            _, flickr_file_name = record['image']['flickr_url'].rsplit('/', maxsplit=1)
            flickr_id, _ = flickr_file_name.split('_', maxsplit=1)
            meta['flickr_full_page'] = 'http://flickr.com/photo.gne?id={}'.format(flickr_id)
        if self.preprocess is not None:
            image, record, more, _ = self.preprocess(image, record, None, None)
            meta = dict(more or {}, **meta)
        if self.target_transforms is not None:
            record = [t(record, meta, None) for t in self.target_transforms]
        return image, record, meta

    def __len__(self):
        return len(self.ids)


class ImageList:
    """Images without annotations: dataset[i] -> (image (h, w, 3) uint8 RGB, [], meta)."""

    def __init__(self, image_paths, preprocess=None):
        self.image_paths, self.preprocess = list(image_paths), preprocess

    def __getitem__(self, index):
        image_path = self.image_paths[index]
        image, anns, meta = read_rgb(image_path), [], {}
        if self.preprocess is not None:
            image, anns, meta, _ = self.preprocess(image, anns, None, None)
        meta = dict(meta or {}, dataset_index=index, file_name=image_path)
        return image, anns, meta

    def __len__(self):
        return len(self.image_paths)


def collate_raw(batch):
    """[(image, record, meta)] of CocoKeypoints items -> (images: the list of raw arrays, joints (N,P,17,4) fp32 padded with zeros to
    the batch's largest person count, n_persons (N,) int32, tables: annotations.MaskTables of the batch, metas)."""
    images = [b[0] for b in batch]
    records = [b[1] for b in batch]
    for im, rec in zip(images, records):
        if tuple(im.shape[:2]) != (rec['height'], rec['width']):
            raise ValueError(f"image {rec.get('image_id')}: decoded size {im.shape[:2]} is not the annotation file's "
                             f"{(rec['height'], rec['width'])}")
    kps = [normalize_annotations(rec) for rec in records]
    n_persons = np.array([len(k) for k in kps], np.int32)
    joints = np.zeros((len(batch), int(n_persons.max(initial=0)), 17, 4), np.float32)
    for i, k in enumerate(kps):
        joints[i, :len(k)] = k
    return images, joints, n_persons, mask_tables(records), [b[2] for b in batch]


def raw_batches(dataset, batch_size):
    """Batches (images, [None] * n, metas) of raw images for evaluate.run_images' raw-uint8 path; metas carry 'image_id' (the
    dataset index for an ImageList)."""
    for first in range(0, len(dataset), batch_size):
        items = [dataset[i] for i in range(first, min(first + batch_size, len(dataset)))]
        metas = [dict(m, image_id=m.get('image_id', m['dataset_index'])) for _, _, m in items]
        yield [im for im, _, _ in items], [None] * len(items), metas
