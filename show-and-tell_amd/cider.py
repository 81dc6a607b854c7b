"""CIDEr on the device: `CiderScorer.compute_score()` of the reference (`pycocoevalcap/cider/cider_scorer.py:93-181`, n = 4,
sigma = 6.0 -- the number `train.py:169-177` keeps `model-best.pth` by) for token-id captions.

    refs, ext = sat.encode_references(tokenized, vocab.word2idx)      # once: words -> ids, fresh ids for words outside the vocabulary
    scorer = sat.CiderScorer(refs)                                    # once: trie + table + reference norms on the device
    mean, scores = scorer.score(ids, image_index, end_id=2)           # per batch: f64 device tensors, nothing synchronised

Captions are ids in an EXTENDED id space: a reference word the vocabulary lacks gets an id of its own >= len(vocab) instead of
`<unk>`, which would merge distinct n-grams and change the document frequencies and the reference norms; with it the score equals
the reference's on the same tokenised strings.  The arithmetic is stated at `sat_cider_score` in include/sat_hip.h; the kernels
are csrc/sat_cider.hip.  There is no CPU path: the host only builds the corpus trie (numpy, at construction)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

ORDERS = 4
MAX_HYP_TOKENS = 64
MAX_REF_TOKENS = 128
_HASH = np.uint64(0x9E3779B97F4A7C15)


def encode_references(tokenized, word2idx):
    """tokenized: per image, per reference, a list of words.  Returns (ids, ext): the same nesting with ids, and `ext`, word2idx
    extended by one fresh id (len(word2idx), len(word2idx) + 1, ... in order of first appearance) per word it does not have."""
    ext = dict(word2idx)
    if ext and (min(ext.values()) < 0 or max(ext.values()) >= 2 ** 31):
        raise ValueError("word2idx ids must lie in [0, 2**31)")
    nxt = max(ext.values()) + 1 if ext else 0
    nxt = max(nxt, len(ext))
    out = []
    for refs in tokenized:
        if isinstance(refs, str) or any(isinstance(r, str) for r in refs):
            raise TypeError("a reference is a list of words (tokenise first), not a string")
        rows = []
        for ref in refs:
            row = []
            for w in ref:
                if not isinstance(w, str):
                    raise TypeError("words must be str, got %r" % (w,))
                if w not in ext:
                    if nxt >= 2 ** 31:
                        raise ValueError("the extended id space passed 2**31")
                    ext[w] = nxt
                    nxt += 1
                row.append(ext[w])
            rows.append(row)
        out.append(rows)
    return out, ext


def table_slot(keys, capacity):
    """the slot a key's probe sequence starts at (the kernels' `cider_slot`): ((key * 0x9E3779B97F4A7C15) >> 32) & (capacity - 1)"""
    keys = np.asarray(keys, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return ((keys * _HASH) >> np.uint64(32)) & np.uint64(capacity - 1)


def min_capacity(n_keys):
    """the smallest table the library takes: a power of two >= 2 * n_keys"""
    cap = 2
    while cap < 2 * n_keys:
        cap *= 2
    return cap


def flatten_references(refs):
    """validate and flatten: (tokens i32 [N], ref_offsets i32 [R+1], image_offsets i32 [I+1]).  Host only."""
    if len(refs) == 0:
        raise ValueError("the corpus has no image")
    tokens, ref_off, img_off = [], [0], [0]
    for i, image in enumerate(refs):
        if len(image) == 0:
            raise ValueError("image %d has no reference caption" % i)
        for ref in image:
            if len(ref) > MAX_REF_TOKENS:
                raise ValueError("a reference of image %d has %d tokens; at most %d are supported" % (i, len(ref), MAX_REF_TOKENS))
            for t in ref:
                if isinstance(t, bool) or not isinstance(t, (int, np.integer)):
                    raise TypeError("reference tokens must be integer ids (see encode_references), got %r" % (t,))
                if not 0 <= t < 2 ** 31:
                    raise ValueError("token id %d of image %d is outside [0, 2**31)" % (t, i))
            tokens.extend(ref)
            ref_off.append(len(tokens))
        img_off.append(len(ref_off) - 1)
    if len(tokens) == 0:
        raise ValueError("every reference caption is empty")
    if len(tokens) >= 2 ** 31:
        raise ValueError("the corpus has 2**31 tokens or more")
    return np.asarray(tokens, dtype=np.int32), np.asarray(ref_off, dtype=np.int32), np.asarray(img_off, dtype=np.int32)


def build_trie(tokens, ref_offsets, image_offsets, orders=ORDERS):
    """The corpus n-grams as trie nodes, order by order with `np.unique` over (parent node, token) pairs: node 0 is the root, node
    j + 1 has key keys[j] = (parent << 32) | token and document frequency df[j] (images whose references hold it).
    Returns (keys u64 [M], df i32 [M], order i8 [M])."""
    tokens = np.asarray(tokens, dtype=np.int64)
    n_refs, n_images = len(ref_offsets) - 1, len(image_offsets) - 1
    ref_len = np.diff(ref_offsets).astype(np.int64)
    ref_of_tok = np.repeat(np.arange(n_refs), ref_len)
    end_of_tok = np.asarray(ref_offsets, dtype=np.int64)[1:][ref_of_tok]             # one past the last token of the position's caption
    image_of_ref = np.repeat(np.arange(n_images), np.diff(image_offsets))
    image_of_tok = image_of_ref[ref_of_tok]
    pos = np.arange(len(tokens))
    parent = np.zeros(len(tokens), dtype=np.int64)            # node of the (k-1)-gram that starts at a position
    keys, dfs, orders_out, base = [], [], [], 0
    for k in range(orders):
        p = pos[pos + k < end_of_tok]
        if len(p) == 0:
            break
        key = ((parent[p] << 32) | tokens[p + k]).astype(np.uint64)
        uniq, inv = np.unique(key, return_inverse=True)
        inv = inv.reshape(-1)
        parent[p] = base + 1 + inv
        pairs = np.unique(inv.astype(np.int64) * n_images + image_of_tok[p])
        keys.append(uniq)
        dfs.append(np.bincount(pairs // n_images, minlength=len(uniq)).astype(np.int32))
        orders_out.append(np.full(len(uniq), k + 1, dtype=np.int8))
        base += len(uniq)
    if base >= 2 ** 31:
        raise ValueError("the corpus has 2**31 distinct n-grams or more")
    return np.concatenate(keys), np.concatenate(dfs), np.concatenate(orders_out)


def _dev(a, device):
    """a numpy array on the device, bit for bit (u64 rides as i64)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(device)


def build_table(keys, capacity=None, device="cuda"):
    """Insert `keys` (u64 [M]) into an open-addressing table on the device; node j + 1 lands beside keys[j].  Returns
    (table_keys i64 [capacity] holding the u64 bits, table_nodes i32 [capacity]).  Reads the kernel's status word once and raises
    RuntimeError when the table filled up or a key came twice."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys.ndim != 1 or len(keys) == 0:
        raise ValueError("keys must be a non-empty vector")
    capacity = min_capacity(len(keys)) if capacity is None else int(capacity)
    if capacity < 2 * len(keys) or capacity & (capacity - 1):
        raise ValueError("capacity must be a power of two >= 2 * len(keys)")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("show-and-tell_amd: the CIDEr table lives on the MI355X; the HIP path has no CPU fallback")
    with torch.cuda.device(device):
        kd = _dev(keys, device)
        tk = torch.empty(capacity, dtype=torch.int64, device=device)
        tn = torch.empty(capacity, dtype=torch.int32, device=device)
        status = torch.empty(1, dtype=torch.int32, device=device)
        L.check(L.load().sat_cider_table_insert(kd.data_ptr(), len(keys), tk.data_ptr(), tn.data_ptr(), capacity, status.data_ptr(),
                                                L.stream()), "sat_cider_table_insert")
        st = int(status.item())              # the one host read of construction
    if st:
        raise RuntimeError("show-and-tell_amd: CIDEr table build failed (status %d:%s%s)"
                           % (st, " table full" if st & 1 else "", " duplicate key" if st & 2 else ""))
    return tk, tn


class CiderScorer:
    """refs: per image, a list of reference captions, each a list of int ids in [0, 2**31) (see `encode_references`).
    Construction validates on the host, builds the n-gram trie with numpy, then the table and the reference norms on the device."""

    def __init__(self, refs, n=4, sigma=6.0, device="cuda"):
        if n != ORDERS:
            raise ValueError("only n = 4 is implemented (the reference's default), got n = %r" % (n,))
        sigma = float(sigma)
        if not (sigma > 0.0 and np.isfinite(sigma)):
            raise ValueError("sigma must be positive and finite")
        tokens, ref_off, img_off = flatten_references(refs)
        keys, df, _ = build_trie(tokens, ref_off, img_off)
        self.n, self.sigma = n, sigma
        self.n_images, self.n_refs, self.n_nodes = len(img_off) - 1, len(ref_off) - 1, len(keys)
        self.device = torch.device(device)
        self.table_keys, self.table_nodes = build_table(keys, None, self.device)         # raises off the GPU
        self.capacity = self.table_keys.numel()
        self.df = _dev(df, self.device)
        self.ref_tokens, self.ref_offsets, self.image_offsets = (_dev(a, self.device) for a in (tokens, ref_off, img_off))
        self.ref_norm = torch.empty(self.n_refs, ORDERS, dtype=torch.float64, device=self.device)
        self._corpus = L.SatCiderCorpus(
            table_keys=self.table_keys.data_ptr(), table_nodes=self.table_nodes.data_ptr(), df=self.df.data_ptr(),
            ref_tokens=self.ref_tokens.data_ptr(), ref_offsets=self.ref_offsets.data_ptr(),
            image_offsets=self.image_offsets.data_ptr(), ref_norm=self.ref_norm.data_ptr(), capacity=self.capacity,
            n_tokens=len(tokens), n_nodes=self.n_nodes, n_refs=self.n_refs, n_images=self.n_images,
            max_ref_tokens=max(1, int(np.diff(ref_off).max())))
        with torch.cuda.device(self.device):
            L.check(L.load().sat_cider_ref_stats(C.byref(self._corpus), self.ref_norm.data_ptr(), L.stream()), "sat_cider_ref_stats")

    def _image_index(self, image_index, B):
        if torch.is_tensor(image_index) and image_index.is_cuda:
            if image_index.dtype not in (torch.int32, torch.int64) or image_index.dim() != 1:
                raise TypeError("image_index must be a vector of int32 or int64")
            idx = image_index.to(torch.int32).contiguous()         # out-of-range entries are clamped by the kernel
        else:
            host = np.asarray(image_index.cpu() if torch.is_tensor(image_index) else image_index)
            if host.ndim != 1 or host.dtype.kind not in "iu":
                raise TypeError("image_index must be a vector of integers")
            if len(host) and (host.min() < 0 or host.max() >= self.n_images):
                raise ValueError("image_index out of range: the corpus has %d images" % self.n_images)
            idx = _dev(host.astype(np.int32), self.device)
        if idx.numel() != B:
            raise ValueError("image_index has %d entries for %d rows" % (idx.numel(), B))
        return idx

    def score(self, ids, image_index, end_id=2, kept=None):
        """ids: int64 [B, T] with contiguous rows (`sample` / `sample_beam`), T <= 64; a 1-D row is one caption.  Row b is scored
        against the references of image image_index[b] and ends at kept[b] (i32 [B] on the device, `kept_tokens`) or, without
        `kept`, in front of its first `end_id`.  Returns (mean f64 [1], scores f64 [B]) on the device; nothing is synchronised."""
        L.require_gpu(ids, "ids")
        if ids.dim() == 1:
            ids = ids.view(1, -1)
        if ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1:
            raise TypeError("ids must be an int64 matrix with contiguous rows")
        if ids.device != self.table_keys.device:
            raise ValueError("ids are on %s, the corpus on %s" % (ids.device, self.table_keys.device))
        B, T = ids.shape
        if B < 1 or T < 1:
            raise ValueError("ids is empty")
        if T > MAX_HYP_TOKENS:
            raise ValueError("rows of %d tokens; at most %d are supported" % (T, MAX_HYP_TOKENS))
        if kept is not None:
            L.require_gpu(kept, "kept")
            if kept.dtype != torch.int32 or kept.dim() != 1 or kept.numel() != B or not kept.is_contiguous():
                raise TypeError("kept must be a contiguous int32 vector with one entry per row")
        idx = self._image_index(image_index, B)
        scores = torch.empty(B, dtype=torch.float64, device=ids.device)
        mean = torch.empty(1, dtype=torch.float64, device=ids.device)
        L.check(L.load().sat_cider_score(C.byref(self._corpus), ids.data_ptr(), ids.stride(0) if B > 1 else T, B, T, L.ptr(kept),
                                         int(end_id), idx.data_ptr(), self.sigma, scores.data_ptr(), mean.data_ptr(), L.stream()),
                "sat_cider_score")
        return mean, scores
