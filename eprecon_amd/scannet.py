"""The ScanNet fragment dataset — mirror of datasets/scannet.py of the reference (ScanNetDataset, :9-172).

    ds = ScanNetDataset(datapath, "test", transforms, nviews=9, n_scales=2)
    sample = ds[i]          # what the transform pipeline of eprecon_amd.transforms takes

<datapath>/all_tsdf_<nviews>_1/fragments_<mode>.pkl lists the fragments (eprecon_amd.generate_gt writes it) and
<datapath>/all_tsdf_<nviews>_1/<scene>/full_*_layer<l>.npz hold the scene's volumes; the frames are read from
<source_path>/<scene>/{color/color_<id>.jpg, depth/depth_<id>.png, pose/pose_<id>.txt, intrinsic/intrinsic_color.txt}.
Same names and item dict as the reference, with two differences: the reference's hard-coded absolute source directory is
the `source_path` argument (default <datapath>/scans, or scans_test in test mode), and the depth PNGs are read with PIL
(the reference uses cv2, which this project does not have).

raw=True hands the frames on as they are decoded — PIL colour images, uint16 depth in millimetres — for
transforms.PrepareViews, which converts them on the device; raw=False gives the reference's host values (PIL colour images
for ResizeImage, float32 depth in metres with everything beyond 3 m zeroed).  A scene's volumes are uploaded once, as a
transforms.SceneVolumes, and kept for up to 50 scenes.
"""
import os
import pickle

import numpy as np

from .scene_io import depth_metres, intrinsic, pose
from .transforms import SceneVolumes

MAX_DEPTH = 3.0       # datasets/scannet.py:62


class ScanNetDataset:
    def __init__(self, datapath, mode, transforms, nviews, n_scales, source_path=None, raw=True, device=None):
        assert mode in ["train", "val", "test"]
        self.datapath = datapath
        self.mode = mode
        self.n_views = nviews
        self.transforms = transforms
        self.tsdf_file = 'all_tsdf_{}_1'.format(self.n_views)
        self.metas = self.build_list()
        self.source_path = source_path or os.path.join(datapath, 'scans_test' if mode == 'test' else 'scans')
        self.n_scales = n_scales
        self.raw = raw
        self.device = device
        self.epoch = None
        self.tsdf_cashe = {}      # scene -> its volume entries of the item dict (the reference's name; main.py clears it per epoch)
        self.max_cashe = 50

    def build_list(self):
        with open(os.path.join(self.datapath, self.tsdf_file, 'fragments_{}.pkl'.format(self.mode)), 'rb') as f:
            return pickle.load(f)

    def __len__(self):
        return len(self.metas)

    def read_cam_file(self, filepath, vid):
        return intrinsic(filepath, 'color').astype(np.float32), pose(filepath, vid)

    def read_img(self, filepath):
        from PIL import Image
        img = Image.open(filepath)
        img.load()            # decode here (a worker thread of the caller's) and let go of the file
        return img

    def read_depth(self, filepath):
        """16-bit PNG in millimetres: as it is (raw), or as float32 metres with everything beyond 3 m zeroed"""
        if not self.raw:
            return depth_metres(filepath, MAX_DEPTH)
        from PIL import Image
        with Image.open(filepath) as im:
            depth_mm = np.asarray(im)
        if depth_mm.dtype != np.uint16:
            depth_mm = depth_mm.astype(np.uint16)         # (PIL's mode "I": the same values as int32)
        return np.ascontiguousarray(depth_mm)

    def read_scene_volumes(self, data_path, scene):
        """{'tsdf_list_full': ...}: the scene's full volumes on the device (with colour and labels in train mode), uploaded
        once.  With device="cpu" asked for by name they stay the reference's host lists, under the reference's four keys
        (RandomTransformSpace takes both forms)."""
        if scene not in self.tsdf_cashe:
            if len(self.tsdf_cashe) > self.max_cashe:
                self.tsdf_cashe = {}
            panoptic = self.mode == 'train'
            if self.device is not None and str(self.device).startswith("cpu"):
                patterns = {'tsdf_list_full': 'full_tsdf_layer{}.npz'}
                if panoptic:
                    patterns.update(rgb_list_full='full_rgb_layer{}.npz', semantic_list_full='full_semantic_layer_interpolate{}.npz',
                                    instance_list_full='full_instance_layer_interpolate{}.npz')
                volumes = {}
                for key, pattern in patterns.items():
                    volumes[key] = []
                    for l in range(self.n_scales + 1):
                        with np.load(os.path.join(data_path, scene, pattern.format(l)), allow_pickle=True) as archive:
                            volumes[key].append(archive['arr_0'])
            else:
                volumes = {'tsdf_list_full': SceneVolumes.load(data_path, scene, panoptic=panoptic, n_scales=self.n_scales,
                                                               device=self.device)}
            self.tsdf_cashe[scene] = volumes
        return self.tsdf_cashe[scene]

    def read_view(self, meta, vid):
        """the file reads of one view: (colour image, depth, intrinsics f32[3,3], extrinsics f64[4,4]).  Touches neither the
        device nor the dataset's state: a caller may run the views of a fragment on threads."""
        scene_dir = os.path.join(self.source_path, meta['scene'])
        img = self.read_img(os.path.join(scene_dir, 'color', 'color_{:d}.jpg'.format(vid)))
        depth = self.read_depth(os.path.join(scene_dir, 'depth', 'depth_{:d}.png'.format(vid)))
        return (img, depth) + self.read_cam_file(scene_dir, vid)

    @staticmethod
    def stack_views(views):
        """read_view() results of a fragment, in order -> (imgs, depth, intrinsics f32[V,3,3], extrinsics f64[V,4,4])"""
        imgs, depth, intrinsics, extrinsics = (list(x) for x in zip(*views))
        return imgs, depth, np.stack(intrinsics), np.stack(extrinsics)

    def read_frames(self, meta):
        return self.stack_views([self.read_view(meta, vid) for vid in meta['image_ids']])

    def make_item(self, idx, frames):
        """the item dict of fragment idx from its read_frames(), through the transforms"""
        meta = self.metas[idx]
        imgs, depth, intrinsics, extrinsics = frames
        items = {
            'imgs': imgs,
            'depth': depth,
            'intrinsics': intrinsics,
            'extrinsics': extrinsics,
            **self.read_scene_volumes(os.path.join(self.datapath, self.tsdf_file), meta['scene']),
            'vol_origin': meta['vol_origin'],
            'scene': meta['scene'],
            'fragment': meta['scene'] + '_' + str(meta['fragment_id']),
            'epoch': [self.epoch],
        }
        if self.transforms is not None:
            items = self.transforms(items)
        return items

    def __getitem__(self, idx):
        return self.make_item(idx, self.read_frames(self.metas[idx]))
