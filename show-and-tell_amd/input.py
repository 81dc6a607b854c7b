"""Host-side input plumbing on either side of the hot path: the batch invariant the kernels rely
on, and an H2D prefetcher so the PCIe copy of batch i+1 hides under the step of batch i (PCIe note).

`collate_batch` keeps the contract of the reference's `collate_fn` (`/root/reference/data_loader.py:48-62`): samples
sorted by caption length, longest first (equal lengths keep their order), images stacked, captions zero-padded into
one int64 matrix, `lengths` as a Python list.  No GPU work happens here.

`ImageTransform` is the reference's per-sample image transform (`main.py:26-36`: RandomCrop / CenterCrop, RandomHorizontalFlip,
ToTensor, Normalize) as ONE kernel on the MI355X: the host hands over the decoded uint8 HWC images (3.06x fewer bytes over PCIe
than the f32 tensor, and no per-sample float work on the host cores) and gets the f32 NCHW batch every encoder entry point takes,
bit for bit what the torchvision transforms compute.  `DevicePrefetcher(..., transform=...)` runs it behind the H2D copy.
"""
import ctypes

import torch


def collate_batch(samples, pin_memory=False):
    """samples: iterable of (image [3,H,W] float tensor, caption 1-D integer tensor, image id).
    Returns (images [B,3,H,W], captions i64 [B,max_len] zero padded, lengths list[int] descending, image ids tuple).
    Images are stacked as they come, whatever their dtype and layout: uint8 [H,W,3] samples (`torch.from_numpy(np.asarray(img))`)
    give the uint8 [B,H,W,3] batch `ImageTransform` / `DevicePrefetcher(transform=...)` take."""
    ordered = sorted(samples, key=lambda s: int(s[1].shape[0]), reverse=True)      # stable, like list.sort(reverse=True)
    if not ordered:
        raise ValueError("empty batch")
    lengths = [int(s[1].shape[0]) for s in ordered]
    if lengths[-1] < 1:
        raise ValueError("empty caption")
    images = torch.stack([s[0] for s in ordered], 0)
    captions = torch.nn.utils.rnn.pad_sequence([s[1].long() for s in ordered], batch_first=True, padding_value=0)
    if pin_memory:
        images, captions = images.pin_memory(), captions.pin_memory()
    return images, captions, lengths, tuple(s[2] for s in ordered)


def collate_on_device(images, flat_captions, lengths, image_ids=None):
    """`collate_fn` (data_loader.py:48-62) with the data movement on the MI355X: `images` f32 [B,3,H,W] and the ragged
    captions (`flat_captions` int64, samples back to back, dataset order) are already in HBM -- e.g. staged by
    `DevicePrefetcher` -- and `lengths` (host ints, dataset order) say where each caption ends.  Returns the reference's
    batch: images in decreasing-length order (ties keep dataset order), captions zero-padded [B, max_len], lengths list,
    image ids tuple.  The order itself is host integer work on lengths the host already holds: no device sync.

    With uint8 images the sort rides along in the transform, and this function is not needed for them:
        order = sorted(range(B), key=lambda i: -lengths[i])          # stable: ties keep dataset order
        images = transform(images_u8, order=order)                   # f32 [B,3,Hc,Wc], longest caption first"""
    from . import _lib as L
    lib = L.load()
    L.require_gpu(images, "images")
    L.require_gpu(flat_captions, "flat_captions")
    lengths = [int(l) for l in lengths]
    B = len(lengths)
    if B == 0 or images.shape[0] != B:
        raise ValueError("one length per image")
    if min(lengths) < 1 or sum(lengths) != flat_captions.numel():
        raise ValueError("lengths must be >= 1 and sum to flat_captions.numel()")
    if images.dtype != torch.float32 or flat_captions.dtype != torch.int64:
        raise TypeError("images float32, captions int64")
    order = sorted(range(B), key=lambda i: -lengths[i])                       # stable: ties keep dataset order
    offs = [0]
    for l in lengths:
        offs.append(offs[-1] + l)
    dev = images.device
    order_d = torch.tensor(order, dtype=torch.int32, device=dev)
    offs_d = torch.tensor(offs, dtype=torch.int64, device=dev)
    tmax = lengths[order[0]]
    caps = torch.empty(B, tmax, dtype=torch.int64, device=dev)
    images = images.contiguous()
    out_im = torch.empty_like(images)
    st = L.stream()
    L.check(lib.sat_collate_captions(flat_captions.contiguous().data_ptr(), offs_d.data_ptr(), order_d.data_ptr(), B, tmax,
                                     caps.data_ptr(), st), "sat_collate_captions")
    L.check(lib.sat_gather_rows_f32(images.data_ptr(), order_d.data_ptr(), B, images[0].numel(), out_im.data_ptr(), st),
            "sat_gather_rows_f32")
    ids = tuple(image_ids[i] for i in order) if image_ids is not None else tuple(order)
    return out_im, caps, [lengths[i] for i in order], ids


class ImageTransform:
    """`main.py:26-36` on the device: uint8 [B,Hs,Ws,3] images (HWC, RGB: what PIL / numpy decode to, e.g. the 256x256 files
    `preprocess.py:90` wrote) -> f32 [B,3,Hc,Wc], cropped, mirrored and normalised by one launch of `sat_image_augment_u8`, bit
    for bit `ToTensor()` + `Normalize(mean, std)` of the cropped / flipped image.

    train=True: RandomCrop(crop_size) + RandomHorizontalFlip() -- `draw` takes top ~ U{0..Hs-Hc}, left ~ U{0..Ws-Wc} and
    flip ~ Bernoulli(0.5) from `generator` (torch's default CPU generator when None); the same seed gives the same sequence.
    train=False: CenterCrop(crop_size), no flip.  In data-parallel runs every rank passes a generator of its own, seeded
    differently per rank (e.g. `torch.Generator().manual_seed(seed + rank)`): ranks that share a seed draw the same crops."""

    def __init__(self, crop_size, train=True, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), generator=None):
        hc, wc = (crop_size, crop_size) if isinstance(crop_size, int) else crop_size
        self.crop_size = (int(hc), int(wc))
        if min(self.crop_size) < 1:
            raise ValueError("crop_size must be positive")
        self.train, self.generator = bool(train), generator
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3:
            raise ValueError("mean and std have one entry per RGB channel")
        # what the kernel reads: the f32 roundings torch.as_tensor(mean, dtype=float32) makes
        self._mean_c, self._std_c = (ctypes.c_float * 3)(*self.mean), (ctypes.c_float * 3)(*self.std)
        if any(v == 0.0 or v != v or abs(v) == float("inf") for v in self._std_c) or any(
                v != v or abs(v) == float("inf") for v in self._mean_c):
            raise ValueError("std must be finite and non-zero in float32, mean finite")

    def _check_source(self, Hs, Ws):
        hc, wc = self.crop_size
        if hc > Hs or wc > Ws:
            raise ValueError("crop %dx%d is larger than the %dx%d source images" % (hc, wc, Hs, Ws))

    def draw(self, B, Hs, Ws):
        """(top, left, flip) for B images of Hs x Ws: a CPU int32 [B,3] tensor"""
        self._check_source(Hs, Ws)
        hc, wc = self.crop_size
        p = torch.zeros(int(B), 3, dtype=torch.int32)
        if self.train:
            g = self.generator
            p[:, 0] = torch.randint(0, Hs - hc + 1, (B,), generator=g, dtype=torch.int32)
            p[:, 1] = torch.randint(0, Ws - wc + 1, (B,), generator=g, dtype=torch.int32)
            p[:, 2] = (torch.rand(B, generator=g) < 0.5).to(torch.int32)
        else:
            p[:, 0], p[:, 1] = int(round((Hs - hc) / 2.)), int(round((Ws - wc) / 2.))        # torchvision's CenterCrop rounding
        return p

    def __call__(self, images_u8, params=None, order=None, out=None):
        """images_u8: uint8 [Bsrc,Hs,Ws,3], contiguous, on the GPU.  params: host int32 [B,3] of (top, left, flip) per OUTPUT
        image (None: `draw`).  order: B host ints, output image b is made from images_u8[order[b]] (None: b, B = Bsrc) -- the
        length sort of `collate_fn` in the same launch.  out: an f32 [B,3,Hc,Wc] contiguous tensor to fill (None: a new one).
        Everything is checked on the host before any GPU call; the parameters are uploaded without a sync and the kernel runs
        on torch's current stream."""
        from . import _lib as L
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8:
            raise TypeError("images must be a uint8 tensor [B,Hs,Ws,3] (the f32 [B,3,H,W] path needs no transform)")
        if images_u8.dim() != 4 or images_u8.shape[3] != 3 or images_u8.shape[0] < 1:
            raise ValueError("images must be [B,Hs,Ws,3] (HWC); got %s" % (tuple(images_u8.shape),))
        Bsrc, Hs, Ws = (int(v) for v in images_u8.shape[:3])
        self._check_source(Hs, Ws)
        hc, wc = self.crop_size
        if order is not None:
            order = torch.as_tensor(order, dtype=torch.int32, device="cpu").reshape(-1)
            if order.numel() < 1 or int(order.min()) < 0 or int(order.max()) >= Bsrc:
                raise ValueError("order must name source images in [0, %d)" % Bsrc)
        B = Bsrc if order is None else order.numel()
        if params is None:
            params = self.draw(B, Hs, Ws)
        else:
            if not isinstance(params, torch.Tensor) or params.dtype != torch.int32 or params.is_cuda:
                raise TypeError("params must be a host int32 tensor [B,3]")
            if tuple(params.shape) != (B, 3):
                raise ValueError("params must be [%d,3] (top, left, flip); got %s" % (B, tuple(params.shape)))
            lo, hi = params.min(0).values.tolist(), params.max(0).values.tolist()
            if lo[0] < 0 or hi[0] > Hs - hc or lo[1] < 0 or hi[1] > Ws - wc or lo[2] < 0 or hi[2] > 1:
                raise ValueError("params out of range: top in [0,%d], left in [0,%d], flip in {0,1}" % (Hs - hc, Ws - wc))
        if out is not None:
            if out.dtype != torch.float32 or tuple(out.shape) != (B, 3, hc, wc) or not out.is_contiguous():
                raise ValueError("out must be a contiguous float32 [%d,3,%d,%d] tensor" % (B, hc, wc))
            if out.device != images_u8.device:
                raise ValueError("out must live on the images' device")
        L.require_gpu(images_u8, "images")
        if not images_u8.is_contiguous():
            raise ValueError("images must be contiguous")
        lib = L.load()
        dev = images_u8.device
        with torch.cuda.device(dev):
            d_params = params.contiguous().pin_memory().to(dev, non_blocking=True)
            d_order = order.pin_memory().to(dev, non_blocking=True) if order is not None else None
            if out is None:
                out = torch.empty(B, 3, hc, wc, dtype=torch.float32, device=dev)
            L.check(lib.sat_image_augment_u8(images_u8.data_ptr(), Bsrc, Hs, Ws, d_params.data_ptr(), L.ptr(d_order), B, hc, wc,
                                             self._mean_c, self._std_c, out.data_ptr(), L.stream()), "sat_image_augment_u8")
        return out


class _Upcoming(list):
    """the list `DevicePrefetcher.upcoming_images()` returns; `.last`: the data ends inside it (`EncoderCNN.prefetch_many`)"""
    last = None


class DevicePrefetcher:
    """Wraps an iterable of (images, captions, lengths, ...) host batches: yields the same tuples with the two tensors
    resident on `device`; the copies of the next `depth` batches run on a side HIP stream while the caller works on the
    current one.  Pinned host tensors make the copies truly asynchronous (`collate_batch(..., pin_memory=True)` or a
    DataLoader with pin_memory).  `upcoming_images()` (inside the loop) returns the device image tensors of the batches
    that follow, in order -- what `TrainStep.step(..., next_images=...)` / `EncoderCNN.prefetch` want for the encoder
    look-ahead; the very same tensor objects are yielded later.

    With `transform` (an `ImageTransform`) a batch whose images are uint8 [B,Hs,Ws,3] crosses PCIe as bytes and is cropped,
    mirrored and normalised on the device, on the copy stream, before its copy-done event: the yielded tuple and
    `upcoming_images()` carry the f32 [B,3,Hc,Wc] tensor exactly as they do for host-transformed batches.  The crop / flip
    parameters are drawn on the host in batch order, so their sequence does not depend on `depth`.  Float batches pass through
    untouched."""

    def __init__(self, batches, device, depth=None, transform=None):
        """depth: batches staged ahead of the one being consumed; None = 6, the encoder's default look-ahead window
        (`EncoderCNN.lookahead_depth`: a smaller depth still works -- `upcoming_images()` tells the look-ahead whether the data
        ends inside the list -- but leaves run slots of the look-ahead empty)"""
        self.batches, self.device = batches, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DevicePrefetcher copies to the MI355X; got device %s" % (device,))
        self.stream = torch.cuda.Stream(self.device)
        self.depth = max(1, int(depth if depth is not None else 6))
        self.transform = transform
        self._queue = []          # [(staged batch tuple, copy-done event)]
        self._done = False        # the wrapped iterable is exhausted: everything that will ever come is staged

    def _draw(self, batch):
        """host half of staging: the transform's (top, left, flip) for a uint8 batch, None for any other"""
        images = batch[0]
        if self.transform is None or images.dtype != torch.uint8:
            return None
        return self.transform.draw(images.shape[0], images.shape[1], images.shape[2])

    def _stage(self, batch):
        return self._upload(batch, self._draw(batch))

    def _upload(self, batch, params):
        images, captions = batch[0], batch[1]
        with torch.cuda.stream(self.stream):
            d_images = images.to(self.device, non_blocking=True)
            if params is not None:
                d_images = self.transform(d_images, params=params)       # same stream as the copy, ahead of the event
            d_captions = captions.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        return (d_images, d_captions) + tuple(batch[2:]), ev

    def _acquire(self, ready, ev):
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)                               # the staged copy is complete before the caller's kernels read it
        for t in ready[:2]:
            t.record_stream(cur)                         # allocator: these blocks are in use on the compute stream

    def upcoming_images(self, wait=False):
        """device image tensors of the staged batches that follow the one just yielded.  Their H2D copies may still be in
        flight.  wait=False (what the encoder look-ahead wants): each tensor carries its copy-done event (`_sat_ready_event`),
        which `EncoderCNN.prefetch` / `prefetch_many` make THEIR side stream wait for -- the caller's compute stream is not held
        up by copies of batches it will only consume later; it waits for a batch's copy when `__iter__` yields that
        batch.  Hand such tensors to nothing but the look-ahead.  wait=True: the current stream waits for every staged copy
        first, so the tensors are safe for ANY use on it."""
        out = _Upcoming()
        out.last = self._done                              # the data ends inside this list: a batch without a partner will not get one
        cur = torch.cuda.current_stream(self.device) if wait else None
        for staged, ev in self._queue:
            if wait:
                cur.wait_event(ev)
                staged[0].record_stream(cur)
            staged[0]._sat_ready_event = ev
            out.append(staged[0])
        return out

    def __iter__(self):
        it = iter(self.batches)
        self._queue = []
        self._done = False
        while True:
            while not self._done and len(self._queue) < self.depth + 1:      # the batch to yield + `depth` copies in flight
                try:
                    self._queue.append(self._stage(next(it)))
                except StopIteration:
                    self._done = True
            if not self._queue:
                return
            ready, ev = self._queue.pop(0)
            self._acquire(ready, ev)
            yield ready
