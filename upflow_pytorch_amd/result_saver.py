"""Saving evaluation results without stalling the evaluation stream: Test_model(save_dir=...) hands every
prediction to a ResultSaver, which

    1. enqueues ops.flow_export on the current stream — the payloads of the requested files, computed on the device;
    2. enqueues asynchronous copies of them into one slot of a small ring of pinned host buffers, and records an event;
    3. hands the slot to a pool of at most `workers` threads, which wait for the event, compress (zlib releases the GIL) and write
           <save_dir>/flow/<name>.png     the KITTI 16-bit flow PNG (a submission directory as it stands on the _test sets)
           <save_dir>/color/<name>.png    the Middlebury colour rendering
           <save_dir>/flo/<name>.flo
           <save_dir>/error/<name>.png    the KITTI devkit's error map against the ground truth (ops.flow_error_image)
       and give the slot back.

The caller never reads a device value.  A full ring blocks submit() until a worker is done with a slot; flush() waits for
everything outstanding and re-raises the first worker exception; close() does the same and ends the pool.

png='device'  moves the compression of the two PNG kinds in front of the copy: step 1 goes on with ops.png_encode on the
`kitti` / `color` payloads, step 2 copies the zlib streams' slots and their lengths instead of the samples, and a worker is left
with the IDAT chunk's CRC and the write (flow_io.write_png_stream).  The files decode to the same samples; their bytes differ from
the host writer's, which is why it is opt-in.

'error' is rendered from the uint16 ground truth — submit(..., gt_occ_u16=, gt_noc_u16=), which Evaluation_bench(device_score=True)
supplies — by its own launch; when it is the only kind saved, ops.flow_export is not called."""
import os
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import torch

from . import ops
from .utils import flow_io

# what can be saved -> (sub-directory, extension, key of ops.flow_export's result; 'error' is ops.flow_error_image's)
KINDS = {'kitti': ('flow', '.png', 'kitti'), 'color': ('color', '.png', 'color'), 'flo': ('flo', '.flo', 'flo'),
         'error': ('error', '.png', 'error')}
_WRITERS = {'kitti': flow_io.write_kitti_png_u16, 'color': flow_io.write_png, 'flo': lambda fn, a: flow_io.write_flo_payload(a, fn),
            'error': flow_io.write_png}


class _Slot(object):
    """Pinned host buffers of one prediction in flight, one per saved kind, kept per shape (KITTI has a handful of frame sizes)."""

    def __init__(self):
        self.buffers = {}

    def buffer(self, kind, like):
        key = (kind, tuple(like.shape))
        b = self.buffers.get(key)
        if b is None:
            b = self.buffers[key] = torch.empty(like.shape, dtype=like.dtype, pin_memory=True)
        return b


class ResultSaver(object):
    def __init__(self, save_dir, save=('kitti',), workers=4, max_rad=None, slots=None, png='host', error_log_colors=True, error_dilate=0):
        save = (save,) if isinstance(save, str) else tuple(save)
        if not save or any(k not in KINDS for k in save):
            raise ValueError('ResultSaver: `save` must name some of %s, got %r' % (sorted(KINDS), save))
        if png not in ('host', 'device'):
            raise ValueError("ResultSaver: `png` must be 'host' or 'device', got %r" % (png,))
        self.png = png
        if isinstance(error_dilate, bool) or not isinstance(error_dilate, int) or not 0 <= error_dilate <= ops.ERROR_DILATE_MAX:
            raise ValueError('ResultSaver: `error_dilate` must be an integer in 0..%d, got %r' % (ops.ERROR_DILATE_MAX, error_dilate))
        self.error_log_colors, self.error_dilate = bool(error_log_colors), error_dilate
        workers = int(workers)
        if workers < 1:
            raise ValueError('ResultSaver: at least one worker thread (got %d)' % workers)
        self.save_dir, self.save, self.max_rad = save_dir, save, max_rad
        for k in save:
            os.makedirs(os.path.join(save_dir, KINDS[k][0]), exist_ok=True)
        self.pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix='upflow-save')    # (never sized by the CPU count)
        n = int(slots) if slots is not None else workers + 2
        self.free = queue.Queue()
        for _ in range(max(n, 1)):
            self.free.put(_Slot())
        self.futures = []
        self.lock = threading.Lock()

    def path(self, kind, name):
        sub, ext, _ = KINDS[kind]
        return os.path.join(self.save_dir, sub, name + ext)

    def submit(self, save_name, predflow, occmask=None, gt_occ_u16=None, gt_noc_u16=None):
        """predflow [B,2,H,W] (any float type) on the GPU, occmask [B,1,H,W] or None -> files named save_name (B = 1) or
        save_name_<i>.  gt_occ_u16 / gt_noc_u16: the payload of the two ground-truth flow PNGs, uint16 [B,H,W,3] on the GPU, read
        by the 'error' kind only.  Returns as soon as the work is enqueued; blocks only while every slot of the ring is in flight."""
        if self.pool is None:
            raise RuntimeError('ResultSaver: closed')
        if 'error' in self.save and (gt_occ_u16 is None or gt_noc_u16 is None):
            raise ValueError("ResultSaver: saving 'error' needs the uint16 ground truth of the pair (gt_occ_u16, gt_noc_u16), which only "
                             "Evaluation_bench(device_score=True) / kitti_2015_test(device_score=True) hands over; the plain path and "
                             "the _test sets have none")
        pred = predflow.detach()
        pred = pred if pred.dtype == torch.float32 else pred.float()
        valid = None
        if occmask is not None:
            valid = occmask.detach().to(device=pred.device, dtype=torch.float32).reshape(pred.shape[0], 1, pred.shape[2], pred.shape[3]).contiguous()
        slot = self.free.get()                                             # a full ring blocks the caller here
        try:
            pred = pred.contiguous()
            exported = [k for k in self.save if k != 'error']
            res = ops.flow_export(pred, valid, max_rad=self.max_rad, **{k: True for k in exported}) if exported else {}
            if 'error' in self.save:
                res['error'] = ops.flow_error_image(pred, gt_occ_u16, gt_noc_u16, log_colors=self.error_log_colors, dilate=self.error_dilate)
            host = {}
            for k in self.save:
                payload = res[KINDS[k][2]]
                if self.png == 'device' and KINDS[k][1] == '.png':
                    streams, lengths = ops.png_encode(payload)
                    _, h, w, c = payload.shape
                    host[k] = (slot.buffer(k + ' streams', streams), slot.buffer(k + ' lengths', lengths), (w, h, 8 * payload.element_size(), c))
                    host[k][0].copy_(streams, non_blocking=True)
                    host[k][1].copy_(lengths, non_blocking=True)
                else:
                    host[k] = slot.buffer(k, payload)
                    host[k].copy_(payload, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
            B = pred.shape[0]
            names = [save_name] if B == 1 else ['%s_%d' % (save_name, i) for i in range(B)]
            fut = self.pool.submit(self._work, slot, event, host, names)
        except BaseException:
            self.free.put(slot)
            raise
        with self.lock:
            self.futures.append(fut)

    def _work(self, slot, event, host, names):
        try:
            event.synchronize()
            for k, buf in host.items():
                if isinstance(buf, tuple):                                      # png='device': the zlib streams and their lengths
                    streams, lengths, (w, h, depth, c) = buf[0].numpy(), buf[1].numpy(), buf[2]
                    for i, name in enumerate(names):
                        n = int(lengths[i])
                        if n < 0:
                            raise RuntimeError('ResultSaver: the device encoder\'s stream of %s did not fit its slot' % self.path(k, name))
                        flow_io.write_png_stream(self.path(k, name), w, h, depth, c, streams[i, :n])
                    continue
                arr = buf.numpy()
                for i, name in enumerate(names):
                    _WRITERS[k](self.path(k, name), arr[i])
        finally:
            self.free.put(slot)

    def flush(self):
        """Wait for every file handed in so far; re-raise the first worker exception (in submission order)."""
        with self.lock:
            futures, self.futures = self.futures, []
        first = None
        for f in futures:
            e = f.exception()
            if e is not None and first is None:
                first = e
        if first is not None:
            raise first

    def close(self):
        if self.pool is None:
            return
        try:
            self.flush()
        finally:
            self.pool.shutdown(wait=True)
            self.pool = None
