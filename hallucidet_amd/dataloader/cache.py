"""HBM-resident dataset cache (`--cache-dataset hbm`): decode every image ONCE, keep the uint8 bytes in one arena per modality on the GPU,
and build each batch with one launch of `ops.batch_gather` from an index list.  From the second epoch on the host opens no image file.

  DeviceDatasetCache.build   walks a Single/MultiModalDetectionDataset once, in index order, through a sequential DataLoader over
                             `dataset[i]` (so the bytes are the ones the uncached path decodes and KAIST's `indices` indirection is
                             honoured), uploads through two pinned buffers per modality into `[n, 3, H, W]` / `[n, 1, H, W]` arenas and
                             keeps the targets as the host dicts `__getitem__` returns;
  CachedLoader               has the length, the batch order and the epoch behaviour of the DataLoader it replaces (the same
                             `ShardedBatchSampler` for training, sequential with drop_last otherwise) and yields `IndexBatch`es: the slot
                             numbers and the host targets of one batch;
  DevicePrefetcher           (dataloader.py) stays the only place that stages: given an IndexBatch it uploads the index vector through its
                             pinned slots and gathers on its staging stream.

Policy: whole units (the train dataset, serving the train and validation subsets; the test dataset), no eviction.  A unit whose decoded
bytes exceed the remaining budget, or whose images do not all have one shape, stays on the DataLoader (`CacheUnavailable` says why).
With several ranks every rank builds its own full copy: the epoch permutation is global, every rank eventually reads every sample.
"""
import time

import torch


class CacheUnavailable(RuntimeError):
    """Why a unit cannot be cached (it then stays on the DataLoader)."""


def cuda_device(device):
    """The concrete GPU the cache lives on; `ValueError` for a CPU device (there is no HBM to cache in)."""
    if device is None or str(device) == "gpu":
        device = "cuda"
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise ValueError("cache='hbm' keeps the decoded dataset in GPU memory: it needs a GPU device (got %s%s)"
                         % (device, "" if device.type != "cuda" else ", and no GPU is visible"))
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def check_cacheable(data_augmentation=None, fixed_transformations=None):
    """A host transform runs per sample and per epoch on the decoded image: its output cannot be cached."""
    for name, t in (("data_augmentation", data_augmentation), ("fixed_transformations", fixed_transformations)):
        if t is not None:
            raise ValueError("cache='hbm' caches the decoded images, a host-side `%s` would have to run on them again in every epoch: pass "
                             "None (the GPU augmentation, --augment reference, composes with the cache)" % name)


def unit_bytes(n, shapes):
    """Bytes of the arenas of a unit of `n` samples whose image groups have the [C, H, W] `shapes`."""
    total = 0
    for s in shapes:
        c, h, w = (int(v) for v in s)
        total += int(n) * c * h * w
    return total


def default_budget(device):
    """Half of the free memory of `device` now."""
    return int(torch.cuda.mem_get_info(device)[0]) // 2


class IndexBatch:
    """One batch of a CachedLoader: the arena slots of its samples and their host targets, one list per image group."""
    __slots__ = ("cache", "indices", "targets")

    def __init__(self, cache, indices, targets):
        self.cache, self.indices, self.targets = cache, indices, targets


class DeviceDatasetCache:
    """arenas: one uint8 [n, C, H, W] device tensor per image group (single-modal: one; multi-modal: RGB, IR); targets: per group the
    list of the n host target dicts; decoded: the number of samples read through the dataset's `__getitem__`."""

    def __init__(self, arenas, targets, decoded=0, fill_seconds=0.0):
        self.arenas, self.targets = tuple(arenas), tuple(targets)
        self.decoded, self.fill_seconds = decoded, fill_seconds
        if len(self.arenas) != len(self.targets) or any(len(t) != len(self) for t in self.targets):
            raise ValueError("DeviceDatasetCache: one target list of %d entries per arena" % len(self))

    def __len__(self):
        return int(self.arenas[0].shape[0])

    @property
    def groups(self):
        return len(self.arenas)

    @property
    def nbytes(self):
        return sum(int(a.numel()) * a.element_size() for a in self.arenas)

    def batch(self, indices):
        indices = [int(i) for i in indices]
        return IndexBatch(self, indices, tuple([t[i] for i in indices] for t in self.targets))

    @classmethod
    def build(cls, dataset, device, num_workers=0, budget_bytes=None, log=None, fill_batch=8):
        """One pass over `dataset` in index order.  The host holds the DataLoader's queue of fill batches and two pinned buffers of
        `fill_batch` images per group, never the dataset.  Raises CacheUnavailable when the unit does not fit `budget_bytes` (known after
        the first fill batch, before anything is allocated) or an image has another shape than the first.  `log`: a callable that gets one
        line about the finished fill."""
        from .dataloader import collate_fn
        device = cuda_device(device)
        n = len(dataset)
        if n == 0:
            raise CacheUnavailable("it is empty")
        t0 = time.perf_counter()
        kw = dict(batch_size=fill_batch, shuffle=False, drop_last=False, collate_fn=collate_fn, num_workers=num_workers)
        if num_workers > 0:
            kw["prefetch_factor"] = 2
        it = iter(torch.utils.data.DataLoader(dataset, **kw))
        arenas, shapes, targets, pinned, pos = None, None, None, {}, 0
        try:
            with torch.cuda.device(device):
                for turn, batch in enumerate(it):
                    groups, k = len(batch) // 2, len(batch[0])
                    if arenas is None:
                        shapes = [tuple(batch[2 * g][0].shape) for g in range(groups)]
                        if any(len(s) != 3 or batch[2 * g][0].dtype != torch.uint8 for g, s in enumerate(shapes)):
                            raise CacheUnavailable("its samples are not uint8 [C, H, W] images")
                        need = unit_bytes(n, shapes)
                        if budget_bytes is not None and need > budget_bytes:
                            raise CacheUnavailable("its %d decoded bytes (%d samples of %s) do not fit in the remaining budget of %d bytes"
                                                   % (need, n, " + ".join("x".join(str(v) for v in s) for s in shapes), budget_bytes))
                        try:
                            arenas = [torch.empty((n,) + s, dtype=torch.uint8, device=device) for s in shapes]
                        except torch.OutOfMemoryError:
                            raise CacheUnavailable("the allocation of its %d bytes failed" % need) from None
                        targets = [[] for _ in range(groups)]
                    for g in range(groups):
                        imgs = batch[2 * g]
                        for im in imgs:
                            if tuple(im.shape) != shapes[g] or im.dtype != torch.uint8:
                                raise CacheUnavailable("its images do not all have one shape (%s and %s)" % (shapes[g], tuple(im.shape)))
                        slot = pinned.get((g, turn & 1))
                        if slot is None:
                            slot = pinned[(g, turn & 1)] = [torch.empty((fill_batch,) + shapes[g], dtype=torch.uint8).pin_memory(), None]
                        else:
                            slot[1].synchronize()              # the copy that last read this buffer has finished
                        torch.stack(list(imgs), out=slot[0][:k])
                        arenas[g][pos:pos + k].copy_(slot[0][:k], non_blocking=True)
                        slot[1] = torch.cuda.Event()
                        slot[1].record(torch.cuda.current_stream(device))
                        targets[g].extend(_own(t) for t in batch[2 * g + 1])
                    pos += k
                torch.cuda.synchronize(device)
        finally:
            del it              # ends the fill workers
        if pos != n:
            raise CacheUnavailable("the walk yielded %d of its %d samples" % (pos, n))
        c = cls(arenas, targets, decoded=pos, fill_seconds=time.perf_counter() - t0)
        if log is not None:
            log("dataset cache: decoded %d samples into %.1f MB of GPU memory in %.2f s (%d fill workers)"
                % (pos, c.nbytes / 1e6, c.fill_seconds, num_workers))
        return c


def _own(target):
    """A target dict whose tensors own their storage (a worker's tensors sit in shared memory, one file handle each)."""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in target.items()}


def build_units(units, device, num_workers=0, budget_bytes=None, log=None, build=None):
    """units: [(name, dataset), ...] in build order -> {name: DeviceDatasetCache or None}.  Each unit is offered what the units before it
    left of the budget (default: `default_budget(device)` at the start); a unit that cannot be cached costs nothing and is reported by
    one line of `log`."""
    log = log or (lambda *a: None)
    build = build or DeviceDatasetCache.build
    remaining = default_budget(device) if budget_bytes is None else int(budget_bytes)
    out = {}
    for name, ds in units:
        try:
            c = build(ds, device, num_workers=num_workers, budget_bytes=remaining, log=log)
        except CacheUnavailable as e:
            log("dataset cache: the %s unit stays on the DataLoader: %s" % (name, e))
            out[name] = None
            continue
        remaining -= c.nbytes
        out[name] = c
        log("dataset cache: the %s unit is in HBM: %d samples, %d bytes of the budget left" % (name, len(c), remaining))
    return out


class CachedLoader:
    """Stands where `DataLoader(subset, ...)` stood: the same `__len__`, the same batches in the same order.  `subset_indices[p]` is the
    cache slot of position p of the subset.  `batch_sampler` (training: the ShardedBatchSampler the DataLoader would have been given)
    yields lists of positions and advances its epoch on every `__iter__`; None = sequential, drop_last."""

    def __init__(self, cache, subset_indices, batch_size, batch_sampler=None):
        self.cache, self.subset_indices = cache, [int(i) for i in subset_indices]
        self.batch_size, self.batch_sampler = int(batch_size), batch_sampler
        if self.subset_indices and not 0 <= min(self.subset_indices) <= max(self.subset_indices) < len(cache):
            raise IndexError("CachedLoader: a subset index lies outside the cache's %d slots" % len(cache))

    def __len__(self):
        return len(self.batch_sampler) if self.batch_sampler is not None else len(self.subset_indices) // self.batch_size

    def __iter__(self):
        if self.batch_sampler is not None:
            positions = iter(self.batch_sampler)
        else:
            positions = (range(b * self.batch_size, (b + 1) * self.batch_size) for b in range(len(self)))
        for pos in positions:
            yield self.cache.batch([self.subset_indices[p] for p in pos])
