"""On-device input pipeline: the whole image set resident in HBM as uint8, batches gathered on the
device, ToTensor's ``/ 255`` fused into the kernels that read the input image.

What it replaces: ``utils/datasets.py`` ``DSprites.__getitem__`` (:194-213: ``imgs[idx] * 255`` -> ``ToTensor``),
``CelebA.__getitem__`` (:273-291: ``imread`` -> ``ToTensor``) and ``get_dataloaders`` (:46-71:
``DataLoader(dataset, batch_size, shuffle=True, pin_memory=...)`` with ``num_workers=0``) for data that is already in
memory.  At the ~0.75 M images/s of the native training step the reference's per-item Python ``__getitem__`` + fp32
host-to-device copy is three orders of magnitude too slow; a 64x64x3 data set of 202 599 images is 2.5 GB as uint8 (of
288 GB of HBM).

``DeviceImageLoader`` is iterable like the reference's ``DataLoader``: ``len()`` = number of batches (no drop_last: the
last batch may be smaller, datasets.py:67-71), every item is ``(batch, labels)`` with ``batch`` a uint8 ``[B,C,H,W]``
device tensor (pixel values 0..255, NCHW = ToTensor's output order).  The native ``Trainer`` / loss plugins accept
such batches directly (``engine.input``): conv1 forward, conv1 weight gradient and the likelihood target read 1 byte per
pixel and divide by 255 on the fly, bit-identical to ``ToTensor`` followed by the fp32 kernels.
"""
import numpy as np
import torch


def to_uint8_nchw(images):
    """Images as the reference's datasets hold them -> uint8 [N,C,H,W] tensor (host).

    * dSprites ``imgs`` (datasets.py:148,206): [N,H,W] with values {0,1} -> pixels {0,255}, C = 1;
    * HWC uint8 arrays as ``imread`` returns them (datasets.py:284): [N,H,W,C] -> permuted to [N,C,H,W]
      (what ToTensor does per item);
    * already [N,C,H,W] uint8: unchanged."""
    t = torch.as_tensor(np.asarray(images))
    if t.dtype != torch.uint8:
        raise TypeError("expected uint8 pixel data, got %s" % t.dtype)
    if t.dim() == 3:                                   # dSprites: binary [N,H,W]
        if int(t.max()) <= 1:
            t = t * 255                                # datasets.py:206
        return t.unsqueeze(1).contiguous()
    if t.dim() != 4:
        raise ValueError("expected [N,H,W], [N,H,W,C] or [N,C,H,W], got %s" % (tuple(t.shape),))
    if t.shape[-1] in (1, 3) and t.shape[1] not in (1, 3):
        t = t.permute(0, 3, 1, 2)                      # HWC -> CHW (ToTensor)
    return t.contiguous()


class _DatasetView:
    def __init__(self, loader):
        self._loader = loader

    def __len__(self):
        return self._loader.n_images


class DeviceImageLoader:
    """uint8 image set resident on the device + batch iterator (see the module docstring).

    images: anything ``to_uint8_nchw`` accepts, or a uint8 [N,C,H,W] device tensor; labels: optional [N, ...] tensor
    (dSprites ``lat_values``); without labels the second item of a batch is 0 like CelebA's placeholder (datasets.py:291).
    shuffle: the order of an epoch is drawn exactly as ``DataLoader(dataset, batch_size, shuffle=True)`` draws it
    (datasets.py:67-71) -- the iterator's base seed and the RandomSampler's seed from the global CPU generator, then
    ``torch.randperm(n)`` from a generator of its own -- so the same ``torch.manual_seed`` gives the same batches and leaves
    the CPU generator in the same state as the reference's loader (tests/test_host_logic.py).  The permutation is moved to
    the device ONCE per epoch; a batch is one on-device gather.
    rank / world_size: data parallelism (disvae_amd.parallel).  Every rank draws the SAME permutation (the CPU seed is
    shared: FactorVAE's permute_dims needs that anyway) and takes rows [rank*B, (rank+1)*B) of each global batch of
    world_size*B images, the rank order the global-batch estimators assume; ``len()`` counts global batches.  A ragged last
    global batch is split evenly (up to world_size - 1 images of the epoch are dropped so that all ranks see the same
    batch shape, which the collectives require)."""

    def __init__(self, images, batch_size=64, shuffle=True, labels=None, device="cuda", rank=0, world_size=1):
        if isinstance(images, torch.Tensor) and images.is_cuda:
            if images.dtype != torch.uint8 or images.dim() != 4:
                raise TypeError("device image sets must be uint8 [N,C,H,W]")
            self.images = images.contiguous()
        else:
            self.images = to_uint8_nchw(images).to(device)
        self.labels = None if labels is None else torch.as_tensor(labels)
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        if not (0 <= int(rank) < int(world_size)):
            raise ValueError("rank %r outside world_size %r" % (rank, world_size))
        self.rank, self.world_size = int(rank), int(world_size)
        self.dataset = _DatasetView(self)              # ``len(loader.dataset)`` = images, as main.py:201 logs it

    @property
    def n_images(self):
        return self.images.shape[0]

    def _global_batches(self):
        """[(first index into the epoch's order, images per rank)] of every global batch."""
        n, bg = self.n_images, self.batch_size * self.world_size
        out = []
        for i in range(0, n, bg):
            per = min(self.batch_size, (n - i) // self.world_size)
            if per > 0:
                out.append((i, per))
        return out

    def __len__(self):
        """number of batches (training.py:118), the last one possibly smaller."""
        return len(self._global_batches())

    @staticmethod
    def epoch_order(n):
        """The index order ``DataLoader(shuffle=True, num_workers=0)`` iterates an n-item data set in, with the same
        consumption of the global CPU generator (torch/utils/data/dataloader.py: the iterator's base seed;
        sampler.py RandomSampler.__iter__: a seed for a private generator, then randperm)."""
        torch.empty((), dtype=torch.int64).random_()                       # _BaseDataLoaderIter._base_seed (unused here)
        seed = int(torch.empty((), dtype=torch.int64).random_().item())   # RandomSampler.__iter__
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(n, generator=g)

    def __iter__(self):
        dev = self.images.device
        order = order_dev = None
        if self.shuffle:
            order = self.epoch_order(self.n_images)
            order_dev = order.to(dev)                  # ONE host-to-device copy per epoch
        for i, per in self._global_batches():
            lo = i + self.rank * per
            if order is None:
                batch = self.images[lo:lo + per]
                lab = 0 if self.labels is None else self.labels[lo:lo + per]
            else:
                batch = self.images.index_select(0, order_dev[lo:lo + per])   # gather on the device: uint8, B x C x H x W bytes
                lab = 0 if self.labels is None else self.labels[order[lo:lo + per]]
            yield batch, lab


def draw_pair_partners(rows, lat_sizes, k, generator):
    """Partners for the weakly-supervised pair losses (Locatello et al. 2020; models.losses.WeakVaeLoss): for every row of a data
    set that enumerates ``lat_sizes`` in row-major order (a row is sum_j value_j * stride_j, as evaluate.draw_fixed_factor_rows
    has it) the row of an image that differs from it in a few factors of variation and shares the others.

    Only factors with two values or more are eligible (e of them).  k = 1 changes exactly one of them, k >= 2 exactly
    min(k, e), k = -1 a number drawn uniformly from 1 .. max(1, e - 1) per row (at least one eligible factor stays shared when
    there are two).  The changed factors are drawn without replacement, and the new value of a changed factor uniformly among
    its OTHER values: it really changes.  All draws come from ``generator`` (a CPU torch.Generator) in a fixed order -- the
    counts (k = -1 only), one uniform score per (row, eligible factor), one offset per eligible factor in factor order -- so the
    same seed gives the same pairs.

    rows: int64 [n] (any order, repeats allowed) -> (partner_rows int64 [n], changed int64 [n]: bit j set when factor j differs)."""
    sizes = [int(s) for s in lat_sizes]
    K = len(sizes)
    if K > 63:
        raise ValueError("at most 63 factors of variation (the changed-factor mask is one int64), got %d" % K)
    k = int(k)
    if k == 0 or k < -1:
        raise ValueError("k must be -1 (a random number of changed factors) or >= 1, got %d" % k)
    eligible = [j for j, s in enumerate(sizes) if s >= 2]
    e = len(eligible)
    if e == 0:
        raise ValueError("no factor of variation takes two values or more: lat_sizes=%s" % (sizes,))
    rows = torch.as_tensor(rows, dtype=torch.int64, device="cpu").reshape(-1)
    n = rows.numel()
    strides = [int(np.prod(sizes[j + 1:], dtype=np.int64)) for j in range(K)]
    if k == -1:
        count = torch.randint(1, max(1, e - 1) + 1, (n,), generator=generator)
    else:
        count = torch.full((n,), min(k, e), dtype=torch.int64)
    # without replacement: the `count` eligible factors with the smallest scores
    rank = torch.rand(n, e, generator=generator).argsort(dim=1).argsort(dim=1)
    pick = rank < count.view(n, 1)                                        # [n, e]
    partner = rows.clone()
    changed = torch.zeros(n, dtype=torch.int64)
    for col, j in enumerate(eligible):
        value = (rows // strides[j]) % sizes[j]
        offset = torch.randint(1, sizes[j], (n,), generator=generator)    # 1 .. size - 1: uniform over the other values
        new = (value + offset) % sizes[j]
        on = pick[:, col].to(torch.int64)
        partner += on * (new - value) * strides[j]
        changed |= on << j
    return partner, changed


class PairedFactorLoader(DeviceImageLoader):
    """Batches of image PAIRS for WeakVaeLoss out of a device-resident data set that enumerates its factors of variation by row
    number (dSprites, 3D shapes, ...: prod(lat_sizes) images in row-major order of the factor values).

    ``batch_size`` counts PAIRS: an item is ``(batch, changed)`` with ``batch`` uint8 [2 P, C, H, W] -- rows [0, P) the first
    members, rows [P, 2 P) their partners, the layout WeakVaeLoss.fused_step takes -- and ``changed`` int64 [P] on the host, bit j
    set when factor j differs within the pair (a label for diagnostics: the loss does not read it).  ``len()`` is
    ceil(N / batch_size); the last batch may be smaller.

    Per epoch the first members follow ``DeviceImageLoader.epoch_order(N)`` (the reference loader's consumption of the global CPU
    generator), then ONE more ``random_()`` draw of that generator seeds a private generator from which ``draw_pair_partners``
    draws a partner for each of the N images, on the host.  The row numbers of all batches go to the device in one copy; a
    batch is one ``index_select`` of 2 P rows.  ``k``: how many factors a partner changes (draw_pair_partners)."""

    def __init__(self, images, lat_sizes, batch_size=64, k=1, device="cuda"):
        super().__init__(images, batch_size=batch_size, shuffle=True, device=device)
        self.lat_sizes = tuple(int(s) for s in lat_sizes)
        if int(np.prod(self.lat_sizes, dtype=np.int64)) != self.n_images:
            raise ValueError("lat_sizes %s enumerate %d images, the data set has %d"
                             % (self.lat_sizes, int(np.prod(self.lat_sizes, dtype=np.int64)), self.n_images))
        self.k = int(k)
        draw_pair_partners(torch.zeros(0, dtype=torch.int64), self.lat_sizes, self.k, None)     # refuses a bad k / lat_sizes now

    def __iter__(self):
        n = self.n_images
        order = self.epoch_order(n)
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        partner, changed = draw_pair_partners(order, self.lat_sizes, self.k, g)
        spans = self._global_batches()
        index = torch.cat([torch.cat((order[i:i + per], partner[i:i + per])) for i, per in spans])
        index_dev = index.to(self.images.device)           # ONE host-to-device copy per epoch
        for i, per in spans:
            yield self.images.index_select(0, index_dev[2 * i:2 * (i + per)]), changed[i:i + per]


class LabelledFactorLoader(DeviceImageLoader):
    """Batches for SemiSupervisedVaeLoss out of a device-resident data set that enumerates its factors of variation by row number
    (dSprites, 3D shapes, ...: prod(lat_sizes) images in row-major order of the factor values): half of every batch is the
    unlabelled data set, the other half comes from a small labelled subset.

    ``batch_size`` counts the images of ONE half (P): an item is ``(batch, rows)`` with ``batch`` uint8 [2 P, C, H, W] and
    ``rows`` int64 [2 P] on the device -- what SemiSupervisedVaeLoss.fused_step takes as ``labels``.  Rows [0, P) of a batch
    follow ``DeviceImageLoader.epoch_order(N)`` and carry -1 (unlabelled); rows [P, 2 P) cycle through a per-epoch permutation of
    the labelled subset and carry their row numbers, from which the kernels derive the factor values.  ``len()`` is
    ceil(N / batch_size); the last batch may be smaller (both halves shrink alike).

    The labelled subset -- ``n_labelled`` distinct rows -- is drawn ONCE, at construction, from a private generator seeded with
    ``seed``: the same seed gives the same subset whatever the global generator holds.  Per epoch the first halves consume the
    global CPU generator as the reference loader does, then ONE more ``random_()`` draw of it seeds a private generator for the
    subset's permutation (as PairedFactorLoader does for its partners).  The row numbers of all batches go to the device in one
    copy; a batch is one ``index_select`` of 2 P rows."""

    def __init__(self, images, lat_sizes, batch_size=64, n_labelled=1000, seed=0, device="cuda"):
        super().__init__(images, batch_size=batch_size, shuffle=True, device=device)
        self.lat_sizes = tuple(int(s) for s in lat_sizes)
        if int(np.prod(self.lat_sizes, dtype=np.int64)) != self.n_images:
            raise ValueError("lat_sizes %s enumerate %d images, the data set has %d"
                             % (self.lat_sizes, int(np.prod(self.lat_sizes, dtype=np.int64)), self.n_images))
        self.n_labelled = int(n_labelled)
        if not 1 <= self.n_labelled <= self.n_images:
            raise ValueError("n_labelled must lie in 1 .. %d (the images of the data set), got %d" % (self.n_images, self.n_labelled))
        g = torch.Generator()
        g.manual_seed(int(seed))
        self.labelled_rows = torch.randperm(self.n_images, generator=g)[:self.n_labelled].clone()      # int64 [n_labelled], host

    def __iter__(self):
        n = self.n_images
        order = self.epoch_order(n)
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        perm = torch.randperm(self.n_labelled, generator=g)
        labelled = self.labelled_rows[perm][torch.arange(n) % self.n_labelled]     # position j of the epoch: the cycle's j-th row
        spans = self._global_batches()
        index = torch.cat([torch.cat((order[i:i + per], labelled[i:i + per])) for i, per in spans])
        index_dev = index.to(self.images.device)           # ONE host-to-device copy per epoch
        unlabelled = torch.full((self.batch_size,), -1, dtype=torch.int64, device=self.images.device)
        for i, per in spans:
            sel = index_dev[2 * i:2 * (i + per)]
            yield self.images.index_select(0, sel), torch.cat((unlabelled[:per], sel[per:]))
