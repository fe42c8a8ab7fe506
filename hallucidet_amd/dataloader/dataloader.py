"""Input pipeline: the step BEFORE the hot path -- JPEG decode, VOC-XML annotations, list collate -- with the
reference's class names and constructor keywords (src/dataloader/dataloader.py:77-272 SingleModalDetectionDataset /
MultiModalDetectionDataset, src/dataloader/dataloaderPL.py:94-259 Single/MultiModalDataModule, src/utils/utils.py:212-234
open_txt_file / collate_fn / split_dataset, :342-438 get_bbox) for the LLVIP and FLIR-aligned layouts.

MI355X-first differences (values identical, traffic not):
  * samples stay **uint8** from the decoder through collate, pinned host memory and the host->device copy (1 B/px IR,
    3 B/px RGB instead of the reference's fp32/fp64 tensors: 4-8x less PCIe traffic for the 42 MB fp32 batch of
    BASELINE configs[1]); `DevicePrefetcher` converts on the GPU with one fp32 division by 255 -- exactly the value the
    reference computes on the host (`astype(float)/255.0`, correctly rounded either way);
  * the next batch's copy runs on a side stream while the current step computes.
Host-side python: `PIL` decodes (imageio / cv2 / albumentations are not installed offline); a `data_augmentation`
callable with the albumentations call signature is accepted and applied exactly where the reference applies it
(dataloaderPL.py:21-88), `None` skips it.  KAIST (dataloader.py:102-113,210-217): frame lists come from the dataset's own
`{train,test}-all-20-{rgb,ir}.txt`; the reference hard-codes the 1 300 training positions whose annotation is non-empty
("clean empty bbox from annotation") -- here that set is COMPUTED from the annotations by the same criterion (or read from
`<root>/train-indices.txt` when the user supplies one), not stored in the source.

Data parallelism: every rank builds the SAME train / validation split (one seed) and reads the rank-th interleaved shard of
each epoch's permutation (`ShardedBatchSampler`), so an epoch is one pass over the training set across all ranks.
"""
import glob
import os
import xml.etree.ElementTree as ET
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from .. import ops
from . import cache as hc
from .cache import CachedLoader, IndexBatch


# ------------------------------------------------------------------------------------------------ annotations
def _annotation_path(filename, dataset):
    if dataset == 'kaist':       # utils.py:350-351: the xml sits next to the frame
        return filename
    if dataset == 'llvip':       # utils.py:353: <root>/LLVIP/Annotations/<stem>.xml, whatever split folder the image is in
        return os.path.join(filename[:filename.index('LLVIP')], 'LLVIP', 'Annotations', filename.split('/')[-1])
    if dataset == 'flir':        # utils.py:356-357
        return os.path.join(filename.split('/JPEGImages/')[0], 'Annotations', filename.split('/JPEGImages/')[-1]).replace('RGB', 'PreviewData')
    raise Exception("Dataset not supported")


def get_bbox(filename, dataset='llvip', train=False):
    """utils.py:342-438: VOC xml -> {'bboxes': float64 [G,4] xyxy, 'labels': int [G,1]}; only `person`, min/max
    re-ordered, LLVIP keeps boxes with area > 5 px^2, FLIR keeps area > 10 (train) / height > 50 (test)."""
    root = ET.parse(_annotation_path(filename, dataset)).getroot()
    bboxes, labels = [], []
    for obj in root.findall("object"):
        bb = obj.find("bndbox")
        if dataset == 'kaist':   # utils.py:366,387-389: x, y, w, h
            b = [int(bb.find(k).text) for k in ("x", "y", "w", "h")]
            b[2] += b[0]
            b[3] += b[1]
        else:
            b = [int(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")]
        xmin, ymin, xmax, ymax = min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])
        box = [xmin, ymin, xmax, ymax]
        area = abs(xmax - xmin) * abs(ymax - ymin)
        if dataset == 'flir':
            keep = (area > 10.0) if train else (abs(ymax - ymin) > 50.0)
        else:
            keep = area > 5.0
        if keep and obj.find("name").text == "person":
            bboxes.append(box)
            labels.append([1])
    return {"bboxes": np.array(bboxes).astype("float"), "labels": np.array(labels).astype("int")}


def open_txt_file(file_name, path_images):
    with open(file_name, 'r') as f:
        return [os.path.join(path_images, x.strip()) for x in f.readlines()]


def collate_fn(batch):
    return tuple(zip(*batch))


def split_dataset(train_dataset, split_ratio=0.8, seed=123):
    train_size = int(split_ratio * len(train_dataset))
    return torch.utils.data.random_split(train_dataset, [train_size, len(train_dataset) - train_size],
                                         generator=torch.Generator().manual_seed(seed))


def _target(annot):
    return {"boxes": torch.from_numpy(annot["bboxes"]).squeeze().view(-1, 4), "labels": torch.from_numpy(annot["labels"]).view(-1)}


# ------------------------------------------------------------------------------------------------ datasets
class SingleModalDetectionDataset(torch.utils.data.Dataset):
    def __init__(self, dataset, path_images, modality=None, transforms=None, ext=".png", train=True):
        self.modality, self.ext, self.dataset, self.indices = modality, ext, dataset, None
        self.path_images, self.train, self.transforms = path_images, train, transforms
        if dataset == 'llvip':
            sub = 'visible' if modality in ('rgb', 'both') else 'infrared'
            self.list_names = [x.split('.jpg')[0] for x in sorted(glob.glob(os.path.join(path_images, sub, 'train' if train else 'test', '*.jpg')))]
        elif dataset == 'flir':
            names = sorted(open_txt_file(Path(path_images + '/' + ('align_train.txt' if train else 'align_validation.txt')), path_images))
            self.list_names = [os.path.join(path_images, 'JPEGImages', x.split(path_images)[-1] if modality == 'infrared'
                                            else x.split(path_images)[-1].split('PreviewData')[0] + 'RGB') for x in names]
        elif dataset == 'kaist':
            which = 'rgb' if modality in ('rgb', 'both') else 'ir'
            self.list_names = sorted(open_txt_file(Path(path_images + '/' + ('train' if train else 'test') + '-all-20-%s.txt' % which), path_images))
            if train:
                self.indices = self._kaist_nonempty(path_images)
        else:
            raise Exception("Dataset not supported")

    def _kaist_nonempty(self, root):
        """Training positions with at least one kept `person` box (the criterion behind dataloader.py:106)."""
        f = os.path.join(root, 'train-indices.txt')
        if os.path.exists(f):
            return [int(t) for t in open(f).read().replace(',', ' ').split()]
        return [i for i, n in enumerate(self.list_names) if len(get_bbox(n + ".xml", 'kaist', True)["bboxes"]) > 0]

    def __len__(self):
        return len(self.indices) if self.indices is not None else len(self.list_names)

    def _read(self, path, mode):
        """uint8 tensor [C,H,W] (C = 3 for 'RGB', 1 for 'L')."""
        a = np.array(Image.open(path).convert(mode))            # owning, writable copy
        return torch.from_numpy(np.ascontiguousarray(a if a.ndim == 2 else a.transpose(2, 0, 1))).reshape(-1, a.shape[0], a.shape[1])

    def __getitem__(self, index):
        index = self.indices[index] if self.indices is not None else index
        name = self.list_names[index]
        img = self._read(name + self.ext, "RGB" if self.modality == 'rgb' else "L")
        t = _target(get_bbox(name + ".xml", self.dataset, self.train))
        t["path_image"] = name + self.ext
        if self.transforms is not None:
            img = self.transforms(img)
        return img, t


class MultiModalDetectionDataset(SingleModalDetectionDataset):
    """Aligned RGB + IR pairs (dataloader.py:190-272).  Returns (img_rgb u8 [3,H,W], target_rgb, img_ir u8 [1,H,W], target_ir)."""

    def __init__(self, dataset, path_images_rgb, path_images_ir, modality=None, transforms_rgb=None, transforms_ir=None, ext=".png", train=True):
        super().__init__(dataset=dataset, path_images=path_images_rgb, modality=modality, transforms=None, ext=ext, train=train)
        self.list_names_rgb = self.list_names
        if dataset == 'llvip':
            self.list_names_ir = [x.split('.jpg')[0] for x in sorted(glob.glob(os.path.join(self.path_images, 'infrared', 'train' if train else 'test', '*.jpg')))]
        elif dataset == 'kaist':
            self.list_names_ir = sorted(open_txt_file(Path(path_images_ir + '/' + ('train' if train else 'test') + '-all-20-ir.txt'), path_images_ir))
        else:   # flir
            names = sorted(open_txt_file(Path(self.path_images + '/' + ('align_train.txt' if train else 'align_validation.txt')), self.path_images))
            self.list_names_ir = [os.path.join(self.path_images, 'JPEGImages', x.split(self.path_images)[-1]) for x in names]
        if len(self.list_names_ir) != len(self.list_names_rgb):
            raise ValueError("RGB / IR file lists differ in length (%d vs %d)" % (len(self.list_names_rgb), len(self.list_names_ir)))

    def __getitem__(self, index):
        index = self.indices[index] if self.indices is not None else index
        n_rgb, n_ir = self.list_names_rgb[index], self.list_names_ir[index]
        img_rgb = self._read(n_rgb + self.ext, "RGB")
        img_ir = self._read(n_ir + ('.jpeg' if self.dataset == 'flir' else self.ext), "L")
        a_rgb = get_bbox((n_ir if self.dataset == 'flir' else n_rgb) + ".xml", self.dataset, self.train)
        a_ir = get_bbox(n_ir + ".xml", self.dataset, self.train)
        return img_rgb, _target(a_rgb), img_ir, _target(a_ir)

    def get_name(self, index):
        return self.list_names_rgb[index], self.list_names_ir[index]


class DatasetTransform(torch.utils.data.Dataset):
    """dataloaderPL.py:14-91: optional augmentation with the albumentations call signature
    transform(image=HWC u8, bboxes=, labels=, image1=HW u8, bboxes1=, labels1=) -> dict; an augmentation that drops every
    box falls back to the un-augmented targets (:83-85)."""

    def __init__(self, subset, transform=None, modality='single'):
        self.subset, self.transform, self.modality = subset, transform, modality

    def __len__(self):
        return len(self.subset)

    def __getitem__(self, index):
        if self.modality == 'single':
            imgs, targets = self.subset[index]
            return (self.transform(imgs) if self.transform else imgs), targets
        imgs_rgb, t_rgb, imgs_ir, t_ir = self.subset[index]
        if self.transform:
            b_rgb, b_ir = dict(t_rgb), dict(t_ir)
            out = self.transform(image=imgs_rgb.permute(1, 2, 0).numpy().copy(), bboxes=t_rgb['boxes'], labels=t_rgb['labels'],
                                 image1=imgs_ir[0].numpy().copy(), bboxes1=t_ir['boxes'], labels1=t_ir['labels'])
            imgs_rgb = out['image'] if torch.is_tensor(out['image']) else torch.as_tensor(np.asarray(out['image'])).permute(2, 0, 1).contiguous()
            imgs_ir = out['image1'] if torch.is_tensor(out['image1']) else torch.as_tensor(np.asarray(out['image1']))[None]
            t_rgb = {"boxes": torch.as_tensor(np.asarray(out['bboxes'], dtype=np.float32)).view(-1, 4), "labels": torch.as_tensor(np.asarray(out['labels'])).view(-1).long()}
            t_ir = {"boxes": torch.as_tensor(np.asarray(out['bboxes1'], dtype=np.float32)).view(-1, 4), "labels": torch.as_tensor(np.asarray(out['labels1'])).view(-1).long()}
            if len(t_rgb['boxes']) == 0:
                t_rgb, t_ir = b_rgb, b_ir
        return imgs_rgb, t_rgb, imgs_ir, t_ir


# ------------------------------------------------------------------------------------------------ data modules
class ShardedBatchSampler(torch.utils.data.Sampler):
    """Per-rank batches of a data-parallel epoch: ONE permutation per epoch (seed + epoch, identical on every rank), cut to a
    multiple of world * batch (drop_last, dataloaderPL.py:207-216), rank r takes positions r, r+world, ...  World size 1
    degenerates to a shuffled, drop_last loader."""

    def __init__(self, n, batch_size, rank=0, world_size=1, shuffle=True, seed=123):
        self.n, self.batch_size, self.rank, self.world, self.shuffle, self.seed = n, batch_size, rank, world_size, shuffle, seed
        self.epoch = 0

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __len__(self):
        return self.n // (self.world * self.batch_size)

    def __iter__(self):
        if self.shuffle:
            order = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed + self.epoch)).tolist()
        else:
            order = list(range(self.n))
        self.epoch += 1
        per = len(self) * self.batch_size
        mine = order[self.rank:per * self.world:self.world]
        for b in range(len(self)):
            yield mine[b * self.batch_size:(b + 1) * self.batch_size]


def _loader(ds, batch_size, shuffle, num_workers, seed, rank=0, world_size=1):
    kw = dict(collate_fn=collate_fn, num_workers=num_workers, pin_memory=torch.cuda.is_available())
    if num_workers > 0:
        kw["persistent_workers"] = True
    if shuffle:
        kw["batch_sampler"] = ShardedBatchSampler(len(ds), batch_size, rank, world_size, True, seed)
    else:
        kw.update(batch_size=batch_size, shuffle=False, drop_last=True)
    return torch.utils.data.DataLoader(ds, **kw)


def _caches(cache, units, names, device, num_workers, budget_bytes, rank, log, data_augmentation, fixed_transformations):
    """cache = 'none': {} ; 'hbm': {unit name: DeviceDatasetCache or None} (dataloader/cache.py), built in the order of `units`; a unit
    whose name is not in `names` is not built (its loaders stay DataLoaders)."""
    if cache == 'none':
        return {}
    if cache != 'hbm':
        raise ValueError("cache must be 'none' or 'hbm' (got %r)" % (cache,))
    hc.check_cacheable(data_augmentation, fixed_transformations)
    device = hc.cuda_device(device)
    if log is None:
        log = print if rank == 0 else (lambda *a: None)
    unknown = set(names) - {n for n, _ in units}
    if unknown:
        raise ValueError("cache_units names %s; the units are %s" % (sorted(unknown), [n for n, _ in units]))
    units = [(n, ds) for n, ds in units if n in names]
    return hc.build_units(units, device, num_workers=num_workers, budget_bytes=budget_bytes, log=log)


def _unit_loader(cache, indices, ds, batch_size, shuffle, num_workers, seed, rank=0, world_size=1):
    """The loader of one split: the DataLoader over `ds`, or, when the split's unit is cached, the CachedLoader over the unit's slots
    `indices` that yields the same batches."""
    if cache is None:
        return _loader(ds, batch_size, shuffle, num_workers, seed, rank, world_size)
    sampler = ShardedBatchSampler(len(indices), batch_size, rank, world_size, True, seed) if shuffle else None
    return CachedLoader(cache, indices, batch_size, sampler)


class SingleModalDataModule:
    """cache='hbm' (dataloader/cache.py): the train dataset (serving the train and validation subsets) and then the test dataset are
    decoded once into GPU memory on `device`, within `cache_budget_bytes` (default: half of the free memory); the loaders then yield
    index batches that DevicePrefetcher gathers on the GPU.  `cache_units` names the units to build (a script that reads one split only
    builds that one).  `self.caches` maps the built units' names to the cache, or None for a unit that stayed on the DataLoader."""

    def __init__(self, dataset, path_images_train, path_images_test, batch_size=4, num_workers=4, ext='.png', seed=123,
                 split_ratio_train_valid=0.8, modality='rgb', data_augmentation=None, fixed_transformations=None, rank=0, world_size=1,
                 cache='none', cache_budget_bytes=None, device=None, log=None, cache_units=('train', 'test')):
        base = SingleModalDetectionDataset(dataset, path_images_train, modality=modality, transforms=None, ext=ext, train=True)
        te = SingleModalDetectionDataset(dataset, path_images_test, modality=modality, ext=ext, train=False)
        tr, va = split_dataset(base, split_ratio=split_ratio_train_valid, seed=seed)
        c = self.caches = _caches(cache, [("train", base), ("test", te)], cache_units, device, num_workers, cache_budget_bytes, rank, log,
                                  data_augmentation, fixed_transformations)
        self._train = _unit_loader(c.get("train"), tr.indices, DatasetTransform(tr, data_augmentation, 'single'), batch_size, True, num_workers,
                                   seed, rank, world_size)
        self._valid = _unit_loader(c.get("train"), va.indices, DatasetTransform(va, fixed_transformations, 'single'), batch_size, False,
                                   num_workers, seed)
        self._test = _unit_loader(c.get("test"), range(len(te)), te, batch_size, False, num_workers, seed)

    def train_dataloader(self):
        return self._train

    def val_dataloader(self):
        return self._valid

    def test_dataloader(self):
        return self._test


class MultiModalDataModule:
    """cache='hbm': as SingleModalDataModule, one RGB and one IR arena per unit; with `ablation_flag` validation reads the test unit."""

    def __init__(self, dataset, path_images_train_rgb, path_images_train_ir, path_images_test_rgb, path_images_test_ir, batch_size=4,
                 num_workers=4, ext='.png', seed=123, split_ratio_train_valid=0.8, data_augmentation=None, fixed_transformations=None,
                 ablation_flag=False, rank=0, world_size=1, cache='none', cache_budget_bytes=None, device=None, log=None, cache_units=('train', 'test')):
        base = MultiModalDetectionDataset(dataset, path_images_train_rgb, path_images_train_ir, modality="both", ext=ext, train=True)
        te = MultiModalDetectionDataset(dataset, path_images_test_rgb, path_images_test_ir, modality="both", ext=ext, train=False)
        tr, va = split_dataset(base, split_ratio=split_ratio_train_valid, seed=seed)
        c = self.caches = _caches(cache, [("train", base), ("test", te)], cache_units, device, num_workers, cache_budget_bytes, rank, log,
                                  data_augmentation, fixed_transformations)
        self._train = _unit_loader(c.get("train"), tr.indices, DatasetTransform(tr, data_augmentation, 'multimodal'), batch_size, True,
                                   num_workers, seed, rank, world_size)
        self._valid = _unit_loader(c.get("train"), va.indices, DatasetTransform(va, fixed_transformations, 'multimodal'), batch_size, False,
                                   num_workers, seed)
        self._test = _unit_loader(c.get("test"), range(len(te)), te, batch_size, False, num_workers, seed)
        if ablation_flag:
            self._valid = self._test

    def train_dataloader(self):
        return self._train

    def val_dataloader(self):
        return self._valid

    def test_dataloader(self):
        return self._test


# ------------------------------------------------------------------------------------------------ host -> HBM staging
class DevicePrefetcher:
    """Iterates a loader of collated uint8 batches and yields what `training_step` takes -- (imgs_rgb [N,3,H,W] f32 in [0,1],
    targets_rgb, imgs_ir [N,1,H,W] f32, targets_ir) or (imgs, targets) -- resident in HBM.

    Batch i+1 is staged by a helper thread while the main thread issues step i: the uint8 images are stacked straight into one
    of two reusable pinned buffers per image group, copied on a side HIP stream and divided by 255 on the GPU; the per-image target tensors of one key travel as ONE concatenated pinned copy and are split into views on
    the device (a pageable .to(device) per tensor is a blocking copy each: 64 of them per LLVIP batch).

    A `CachedLoader` (dataloader/cache.py, cache='hbm') yields index batches instead: the images are already in HBM, so only the index
    vector travels through the pinned slots and `ops.batch_gather` builds the same float batch out of the cache's arena with one launch
    on the side stream (as uint8 when an augmentation follows); the targets travel exactly as above."""

    def __init__(self, loader, device="cuda", augment=None, geometry=None):
        """augment: a `ReferenceAugmentation` (dataloader/augment.py) or None.  When given, single-modal batches are augmented as
        uint8, before the division by 255: the per-image parameter rows are drawn for (epoch, batch index), travel as one pinned copy
        and `ops.augment_u8` runs on the staging stream (`apply_host` on a CPU device).
        geometry: a `PairedGeometry` (dataloader/geometry.py) or None.  When given, the per-image records are drawn from the batch's
        host targets for (epoch, batch index) and travel as one pinned copy; every image group of the batch (RGB and IR of a paired
        one) is transformed with the same records by `ops.geometry_u8` on the staging stream -- an uploaded uint8 batch, or the cache's
        arena directly for an index batch -- and the boxes are transformed on the host before their upload.  The kernel's float output
        is the IEEE quotient b / 255; with `augment` as well the geometry yields uint8, the photometric set follows, then the IEEE
        division.  On a CPU device `geometry.apply_host` computes the same bytes."""
        self.augment, self._batch, self._aug_ws = augment, -1, None
        self.geometry = geometry
        self.loader, self.device = loader, torch.device(device)
        self.cuda = self.device.type == "cuda"
        if self.cuda and self.device.index is None:          # the staging thread needs the concrete device
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(device=self.device) if self.cuda else None
        self._slots = {}            # (group, parity) -> [pinned buffer, event of the last copy out of it]
        self._turn = 0

    def __len__(self):
        return len(self.loader)

    def _pinned(self, key, shape, dtype):
        slot = self._slots.get(key)
        if slot is None or slot[0].shape != shape or slot[0].dtype != dtype:
            slot = self._slots[key] = [torch.empty(shape, dtype=dtype).pin_memory(), None]
        elif slot[1] is not None:
            slot[1].synchronize()                      # the copy that last read this buffer has finished
        return slot

    def _upload(self, key, pieces, stack):
        """pieces: CPU tensors; stacked (images) or concatenated along dim 0 (targets) into a pinned slot, one async copy."""
        if not self.cuda:
            return torch.stack(pieces) if stack else torch.cat(pieces)
        shape = ((len(pieces),) + tuple(pieces[0].shape)) if stack else ((sum(int(p_.shape[0]) for p_ in pieces),) + tuple(pieces[0].shape[1:]))
        slot = self._pinned((key, self._turn & 1), torch.Size(shape), pieces[0].dtype)
        if stack:
            torch.stack(pieces, out=slot[0])
        elif shape[0]:
            torch.cat(pieces, out=slot[0])
        dev = slot[0].to(self.device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))
        return dev

    def _stage(self, batch):
        def imgs(g, seq, augment=None):
            seq = list(seq)
            if seq and seq[0].is_cuda:
                u8 = torch.stack(seq)
            else:
                u8 = self._upload(("img", g), seq, True)
            if rows_host is not None:
                if u8.dtype != torch.uint8:
                    raise TypeError("DevicePrefetcher: the geometric augmentation takes uint8 images (got %s)" % u8.dtype)
                if tuple(u8.shape[-2:]) != (H, W):
                    raise ValueError("DevicePrefetcher: the geometric augmentation needs one image size per batch (%s and %s)"
                                     % ((H, W), tuple(u8.shape[-2:])))
                if not u8.is_cuda:
                    from .geometry import apply_host as geometry_host
                    u8 = geometry_host(u8, rows_host)
                elif augment is None:
                    return ops.geometry_u8(u8, rows_dev, mode="f32_ieee")
                else:
                    u8 = ops.geometry_u8(u8, rows_dev, mode="u8")
            return finish(g, u8, augment)

        def gathered(g, idx, idx_host, augment=None):
            """image group g of an IndexBatch (dataloader/cache.py): one gather launch out of the cache's arena on the staging stream"""
            arena = batch.cache.arenas[g]
            if rows_host is not None:
                if tuple(arena.shape[-2:]) != (H, W):
                    raise ValueError("DevicePrefetcher: the geometric augmentation needs one image size per batch (%s and %s)"
                                     % ((H, W), tuple(arena.shape[-2:])))
                if augment is None:
                    return ops.geometry_u8(arena, rows_dev, idx=idx, idx_host=idx_host, mode="f32_ieee")
                return finish(g, ops.geometry_u8(arena, rows_dev, idx=idx, idx_host=idx_host, mode="u8"), augment)
            if augment is None:
                return ops.batch_gather(arena, idx, "f32_default", idx_host=idx_host)
            return finish(g, ops.batch_gather(arena, idx, "u8", idx_host=idx_host), augment)

        def finish(g, u8, augment):
            if augment is not None:
                if u8.dtype != torch.uint8:
                    raise TypeError("DevicePrefetcher: the augmentation takes uint8 images (got %s)" % u8.dtype)
                rows = augment.params_for(u8.shape[0], self._batch)
                if u8.is_cuda:
                    need = ops.augment_ws_bytes(u8.shape)
                    if self._aug_ws is None or self._aug_ws.numel() < need:       # one workspace: every call runs on the staging stream
                        self._aug_ws = torch.empty((need,), dtype=torch.uint8, device=u8.device)
                    u8 = ops.augment_u8(u8, self._upload(("aug", g), [rows], False), ws=self._aug_ws)
                    # a tensor divisor: the IEEE division the host path computes (a Python-scalar divisor is a multiplication by
                    # fp32(1/255) on the GPU, up to one ulp away), so both devices yield the same floats
                    return u8.float().div_(torch.full((), 255.0, device=u8.device))
                from .augment import apply_host
                u8 = apply_host(u8, rows)
            return u8.float().div_(255.0) if u8.dtype == torch.uint8 else u8.float()

        def tgts(g, seq):
            seq = list(seq)
            if rows_host is not None:
                seq = transform_targets(rows_host, seq, H, W)
            out = [dict(t) for t in seq]
            keys = [k for k, v in seq[0].items() if torch.is_tensor(v)] if seq else []
            for k in keys:
                vals = [t[k] for t in seq]
                same = all(torch.is_tensor(v) and v.dim() >= 1 and not v.is_cuda and v.dtype == vals[0].dtype and v.shape[1:] == vals[0].shape[1:] for v in vals)
                if same:
                    flat = self._upload(("tgt", g, k), vals, False)
                    for o, part in zip(out, flat.split([int(v.shape[0]) for v in vals])):
                        o[k] = part
                else:
                    for o, v in zip(out, vals):
                        o[k] = v.to(self.device, non_blocking=True)
            return out
        multi = "DevicePrefetcher: the augmentation is defined for single-modal (image, target) batches only; the reference's HalluciDet " \
                "training has none"
        rows_host = rows_dev = None
        H = W = 0
        if self.geometry is not None:
            from .geometry import check_rows, transform_targets
            if isinstance(batch, IndexBatch):
                groups, (H, W) = batch.targets, batch.cache.arenas[0].shape[-2:]
            else:
                groups, (H, W) = [batch[i] for i in range(1, len(batch), 2)], batch[0][0].shape[-2:]
            H, W = int(H), int(W)
            rows_host = check_rows(self.geometry.params_for(groups, H, W, self._batch), len(groups[0]), H, W, "DevicePrefetcher")
            rows_dev = self._upload(("geo", 0), [rows_host], False)
        if isinstance(batch, IndexBatch):
            if not self.cuda:
                raise RuntimeError("DevicePrefetcher: an index batch of the HBM dataset cache can only be staged on the GPU")
            idx_host = torch.tensor(batch.indices, dtype=torch.int64)
            idx = self._upload(("idx", 0), [idx_host], False)
            if batch.cache.groups == 2:
                if self.augment is not None:
                    raise ValueError(multi)
                return gathered(0, idx, idx_host), tgts(0, batch.targets[0]), gathered(1, idx, idx_host), tgts(1, batch.targets[1])
            return gathered(0, idx, idx_host, self.augment), tgts(0, batch.targets[0])
        if len(batch) == 4:
            if self.augment is not None:
                raise ValueError(multi)
            return imgs(0, batch[0]), tgts(0, batch[1]), imgs(1, batch[2]), tgts(1, batch[3])
        return imgs(0, batch[0], self.augment), tgts(0, batch[1])

    def __iter__(self):
        it = iter(self.loader)
        self._batch = -1

        def fetch():
            try:
                b = next(it)
            except StopIteration:
                return None
            self._turn += 1
            self._batch += 1
            if self.stream is None:
                return self._stage(b)
            torch.cuda.set_device(self.device)
            with torch.cuda.stream(self.stream):
                staged = self._stage(b)
                ready = torch.cuda.Event()
                ready.record(self.stream)
            return staged, ready

        def tensors(x):
            if torch.is_tensor(x):
                yield x
            elif isinstance(x, dict):
                for v in x.values():
                    yield from tensors(v)
            elif isinstance(x, (list, tuple)):
                for v in x:
                    yield from tensors(v)
        if self.stream is None:
            nxt = fetch()
            while nxt is not None:
                cur, nxt = nxt, None
                yield cur
                nxt = fetch()
            return
        # one staging thread: batch i+1 is collated, stacked into pinned memory and enqueued on the side stream while the main
        # thread issues the launches of step i (stack / cat / memcpy release the GIL)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1, thread_name_prefix="hd-stage") as pool:
            fut = pool.submit(fetch)
            while True:
                got = fut.result()
                if got is None:
                    return
                cur, ready = got
                main = torch.cuda.current_stream(self.device)
                main.wait_event(ready)
                for t in tensors(cur):
                    if t.is_cuda:
                        t.record_stream(main)
                fut = pool.submit(fetch)
                yield cur
