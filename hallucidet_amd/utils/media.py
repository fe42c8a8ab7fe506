"""Detection media: the reference's logged panels (train_hallucidet.py:265-280, 309-320, 403-410; train_detector.py:194, 245, 302 --
commented out upstream) as PNG files, rendered on the GPU.

A panel is one batch rendered as ONE uint8 image by `ops.media_render` (hd_media_render: torchvision's make_grid layout; raw panels
quantised as save_image does, "det" panels min-max normalised with ground truths in yellow and detections above the threshold in red,
as Utils.plot_each_image draws them without its text labels).  `MediaWriter.log` issues the render on the current stream, copies the
canvas to a pinned host buffer on a side stream behind an event, and hands it to one worker thread that waits for the copy and encodes
the PNG: the step's thread never waits for the GPU or for the encoder (unless 32 canvases are already queued: back-pressure).
"""
import os
import queue
import threading

import torch

from .. import ops

_QUEUE_DEPTH = 32          # canvases in flight before log() blocks
_PNG_COMPRESS = 1          # zlib level of the encoder: lossless at any level; 1 keeps a 4 100 x 5 100 grid well under a second


_SIDE = {}                 # device -> the copy stream every writer of the process shares


def _side_stream(device):
    """The stream of the D2H copies.  One per device and process, and taken from the HIGH-priority pool: torch hands out the 32 streams
    of a priority round-robin, and the graph captures of the training step (segmentation_models/unet.py, det_graph.py) and the
    prefetcher draw theirs from the default pool -- a writer that took one there would change which of them end up sharing a queue."""
    key = torch.device(device)
    if key.index is None:
        key = torch.device("cuda", torch.cuda.current_device())
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=key, priority=-1)
    return _SIDE[key]


def pad_detections(detections, device):
    """A step's detections as (boxes [N, P, 4], scores [N, P] float32, count [N] int32) on `device` without a host sync: a
    `LazyDetections` that still holds its padded tensors hands them over; per-image lists are padded from their shapes."""
    from ..metrics.device import _pad_list
    pad = detections.padded() if hasattr(detections, "padded") else None
    if pad is not None:
        b, s, _, c = pad
        n = int(c.shape[0])
        P = int(s.shape[1]) if s.dim() == 2 else 0
        return b.reshape(n, P, 4).to(device), s.reshape(n, P).to(device, torch.float32), c.reshape(n).to(device, torch.int32)
    dets = list(detections)
    wide = any(d["boxes"].dtype == torch.float64 for d in dets)
    b, c = _pad_list([d["boxes"] for d in dets], (4,), torch.float64 if wide else torch.float32, device)
    s, _ = _pad_list([d["scores"] for d in dets], (), torch.float32, device)
    return b, s, c


def pad_targets(targets, device):
    """Ground truths (list of dicts with 'boxes') as (boxes [N, Q, 4] float64, count [N] int32) on `device`, padded from their shapes."""
    from ..metrics.device import _pad_list
    return _pad_list([t["boxes"] for t in targets], (4,), torch.float64, device)


def render_panel(batch, mode, detections=None, targets=None, threshold=0.5, nrow=8):
    """One panel -> uint8 [CH, CW, 3] on the batch's device (GPU: hd_media_render; CPU: its numpy twin)."""
    x = ops.as_dense_planes_f32(batch.detach())
    if x.dim() == 4 and x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)              # a one-plane IR batch: read in place through its stride-0 channel view
    dev = x.device
    det = pad_detections(detections, dev) if detections is not None else None
    gt = pad_targets(targets, dev) if targets is not None else None
    fn = ops.media_render if x.is_cuda else ops.media_render_host
    return fn(x, mode, det=det, gt=gt, threshold=threshold, nrow=nrow)


class MediaWriter:
    """Writes DIR/{split}/epoch{E:03d}_batch{B:05d}_{panel}.png for the batches `wants` selects.

    every / offset: the reference's cadence `batch_idx % every == offset` (100 and 1 there); the offset is taken modulo `every`, so
    every=1 selects every batch.  max_batches: stop after that many batches per (split, epoch).  Only rank 0 writes."""

    def __init__(self, dirpath, every=100, offset=1, threshold=0.5, nrow=8, max_batches=None, rank=0):
        if int(every) < 1:
            raise ValueError("MediaWriter: every must be >= 1 (got %r)" % (every,))
        import PIL.Image  # noqa: F401  (fail at construction, not in the worker)
        self.dirpath, self.every, self.offset = str(dirpath), int(every), int(offset)
        self.threshold, self.nrow, self.max_batches, self.rank = float(threshold), int(nrow), max_batches, int(rank)
        self._seen = {}                   # (split, epoch) -> batches written
        self._jobs = queue.Queue(maxsize=_QUEUE_DEPTH)
        self._free = queue.SimpleQueue()  # pinned host buffers the worker has finished with
        self._worker = None
        self._error = None
        self._side = None
        self._closed = False

    def wants(self, batch_idx):
        return self.rank == 0 and int(batch_idx) % self.every == self.offset % self.every

    def path(self, split, epoch, batch_idx, panel):
        return os.path.join(self.dirpath, str(split), "epoch%03d_batch%05d_%s.png" % (int(epoch), int(batch_idx), panel))

    # ------------------------------------------------------------------ step thread
    def _raise_pending(self):
        err, self._error = self._error, None
        if err is not None:
            raise RuntimeError("MediaWriter: the encoder thread failed: %r" % (err,)) from err

    def _pinned(self, nbytes):
        """A pinned host buffer of at least `nbytes`: one the worker has handed back (its copy completed and its PNG is written), else new."""
        kept = []
        buf = None
        while buf is None:
            try:
                b = self._free.get_nowait()
            except queue.Empty:
                break
            if b.numel() >= nbytes:
                buf = b
            else:
                kept.append(b)
        for b in kept:
            self._free.put(b)
        return buf if buf is not None else torch.empty((nbytes,), dtype=torch.uint8).pin_memory()

    def log(self, split, epoch, batch_idx, panels):
        """panels: {name: (batch, mode, detections | None, targets | None)}; rendered on the current stream, written by the worker."""
        self._raise_pending()
        if self.rank != 0 or self._closed:
            return
        key = (str(split), int(epoch))
        if self.max_batches is not None and self._seen.get(key, 0) >= int(self.max_batches):
            return
        self._seen[key] = self._seen.get(key, 0) + 1
        if self._worker is None:
            self._worker = threading.Thread(target=self._run, name="media-writer", daemon=True)
            self._worker.start()
        for name, (batch, mode, detections, targets) in panels.items():
            canvas = render_panel(batch, mode, detections, targets, threshold=self.threshold, nrow=self.nrow)
            path = self.path(split, epoch, batch_idx, name)
            if not canvas.is_cuda:
                self._jobs.put((path, canvas.numpy(), None, None))
                continue
            if self._side is None:
                self._side = _side_stream(canvas.device)
            rendered = torch.cuda.Event()
            rendered.record(torch.cuda.current_stream(canvas.device))
            host = self._pinned(canvas.numel())
            view = host[:canvas.numel()].view(canvas.shape)
            with torch.cuda.stream(self._side):
                self._side.wait_event(rendered)
                view.copy_(canvas, non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(self._side)
            canvas.record_stream(self._side)
            self._jobs.put((path, view.numpy(), copied, host))

    # ------------------------------------------------------------------ worker thread
    def _run(self):
        from PIL import Image
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            path, arr, copied, host = job
            try:
                if copied is not None:
                    copied.synchronize()
                if self._error is None:          # after a failure: drain the queue (buffers come back), write nothing more
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    Image.fromarray(arr).save(path, format="PNG", compress_level=_PNG_COMPRESS)
            except BaseException as e:           # surfaces in the next log() / in close()
                self._error = e
            finally:
                if host is not None:
                    self._free.put(host)
                self._jobs.task_done()

    def flush(self):
        """Wait until every queued panel has been written (or has failed)."""
        if self._worker is not None:
            self._jobs.join()

    def close(self):
        """Wait for the queued panels, stop the worker, re-raise what it raised."""
        if not self._closed:
            self._closed = True
            if self._worker is not None:
                self._jobs.put(None)
                self._worker.join()
                self._worker = None
        self._raise_pending()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
