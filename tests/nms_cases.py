"""Deterministic inputs that drive the batched NMS kernels (mcaq_nms.h) to
their branch edges, and the numpy helpers that prove - with the oracle alone -
that an input reaches the branch it was built for (tests/test_nms_cases_cpu.py)
before the GPU comparison (tests/test_nms_edges_gpu.py) relies on it.

Every builder returns `(pred, kwargs)`: a (B, 4+nc, N) fp32 prediction and the
keyword arguments of `oracle.nms_oracle.non_max_suppression` (conf_thres,
iou_thres, max_det, agnostic, max_nms).  Candidates are written as a
*sequence*: a list of xywh boxes in the order the score sort must produce
(scores fall with the position, equal inside a tie run), scattered over the
anchors by a seeded permutation, so the sort has real work to do and every
expected position is known by construction.  All coordinates are small
integers or halves: box corners, areas and intersections are exact in fp32.

Imports numpy and oracle.nms_oracle only."""
import numpy as np

from oracle import nms_oracle as NO

F32 = np.float32

LDS_KEYS = 8192      # mcaq_nms.h NMS_LDS_KEYS
LDS_KEPT = 1024      # mcaq_nms.h NMS_LDS_KEPT
CHUNK = 256          # mcaq_nms.h NMS_CHUNK
CONF = 0.25
IOU = 0.45
LOW = F32(0.0625)    # score of an anchor that is no candidate


# ---------------------------------------------------------------- numpy helpers
def candidate_counts(pred, conf_thres):
    """Candidates per image as the oracle counts them (max class score > conf;
    a NaN class score makes the maximum NaN and drops the anchor)."""
    pred = np.asarray(pred, F32)
    if pred.shape[2] == 0:
        return np.zeros(pred.shape[0], np.int64)
    with np.errstate(invalid="ignore"):
        return (pred[:, 4:].max(1) > F32(conf_thres)).sum(1).astype(np.int64)


def sorted_candidates(img, conf_thres):
    """One image (4+nc, N): anchor indices of its candidates in the order the
    NMS walks them (score descending, anchor ascending on ties), their scores,
    classes and xyxy boxes."""
    img = np.asarray(img, F32)
    with np.errstate(invalid="ignore"):
        score = img[4:].max(0)
        anchors = np.nonzero(score > F32(conf_thres))[0]
    order = anchors[np.argsort(-score[anchors], kind="stable")]
    return order, score[order], img[4:, order].argmax(0), NO.xywh2xyxy(img[:4, order].T)


def iou_matrix(a, b):
    """Pairwise IoU of xyxy boxes a (n, 4) against b (m, 4) with the oracle's
    fp32 op order (NO.nms): inter / ((area_a + area_b) - inter)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    xx1 = np.maximum(a[:, None, 0], b[None, :, 0])
    yy1 = np.maximum(a[:, None, 1], b[None, :, 1])
    xx2 = np.minimum(a[:, None, 2], b[None, :, 2])
    yy2 = np.minimum(a[:, None, 3], b[None, :, 3])
    inter = np.maximum(F32(0), xx2 - xx1) * np.maximum(F32(0), yy2 - yy1)
    return (inter / ((aa[:, None] + ab[None, :]) - inter)).astype(F32)


def kept_vs_suppressed(img, conf_thres, iou_thres, max_wh=7680, agnostic=False):
    """The oracle's greedy pass over one image without a max_det cut.  Returns
    (kept, sup, iou): sorted positions of the kept and of the suppressed
    candidates, and iou[k, s] of kept box k against suppressed candidate s
    (offset boxes, as the suppression sees them)."""
    order, score, cls, box = sorted_candidates(img, conf_thres)
    off = box + (cls.astype(F32) * F32(0 if agnostic else max_wh))[:, None]
    kept = NO.nms(off, score, iou_thres)          # already sorted: indices are positions
    sup = np.setdiff1d(np.arange(len(order)), kept)
    return kept, sup, iou_matrix(off[kept], off[sup])


def nms_non_greedy(boxes, scores, iou_thres):
    """NOT an NMS anyone ships: every higher-scored overlapping box suppresses,
    alive or not.  An input on which this differs from NO.nms contains a chain
    A > B > C (A kills B, B would kill C, A does not) - the greedy liveness the
    kernel's matrix resolver has to honour."""
    boxes = np.asarray(boxes, F32)
    order = np.argsort(-np.asarray(scores, F32), kind="stable")
    iou = iou_matrix(boxes[order], boxes[order]).astype(np.float64) > np.float64(iou_thres)
    dead = np.triu(iou, 1).any(0)                 # some earlier box overlaps
    return order[~dead].astype(np.int64)


def nms_scalar(boxes, scores, iou_thres):
    """Second, independent restatement of the greedy NMS alone: a double loop
    in plain Python over np.float32 scalars (torchvision's CPU kernel shape:
    for each live i in score order, mark every later j with IoU > thr).  Pins
    NO.nms against a slip in its vectorisation; small inputs only."""
    n = len(scores)
    b = [[F32(v) for v in row] for row in boxes]
    s = [F32(v) for v in scores]
    order = sorted(range(n), key=lambda i: (-float(s[i]), i))
    area = [(r[2] - r[0]) * (r[3] - r[1]) for r in b]
    dead = [False] * n
    keep = []
    for p, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(i)
        for j in order[p + 1:]:
            if dead[j]:
                continue
            xx1, yy1 = max(b[i][0], b[j][0]), max(b[i][1], b[j][1])
            xx2, yy2 = min(b[i][2], b[j][2]), min(b[i][3], b[j][3])
            w, h = max(F32(0), F32(xx2 - xx1)), max(F32(0), F32(yy2 - yy1))
            inter = F32(w * h)
            ovr = F32(inter / F32(F32(area[i] + area[j]) - inter))
            if float(ovr) > float(iou_thres):
                dead[j] = True
    return np.asarray(keep, np.int64)


# ---------------------------------------------------------------- building blocks
def lattice(idx, cols=64, size=16.0):
    """Pairwise disjoint xywh boxes: cell `idx` of a 20-pixel lattice."""
    idx = np.asarray(idx, np.int64)
    out = np.empty((idx.size, 4), F32)
    out[:, 0] = 20 * (idx % cols) + 10
    out[:, 1] = 20 * (idx // cols) + 10
    out[:, 2:] = size
    return out


def near_dup(idx, cols=64, size=15.0):
    """A box concentric with lattice cell idx: IoU 15^2/16^2 = 0.879 with it,
    0 with every other cell and every other cell's duplicates."""
    return lattice(idx, cols, size)


def seq_scores(n, run=1):
    """n scores falling with the position, equal inside runs of `run`:
    0.99 - (p // run) * 2^-14, distinct fp32 values well above CONF."""
    s = F32(0.99) - (np.arange(n) // run).astype(F32) * F32(2.0 ** -14)
    assert s.dtype == F32 and s.min() > 0.4 and (np.diff(s[::run]) < 0).all()
    return s


def place(boxes, scores, N, nc=1, cls=None, seed=0, anchors=None):
    """One image (4+nc, N) whose sorted candidate order is exactly `boxes` /
    `scores` (non-increasing).  Candidate p sits at anchors[p], a seeded
    permutation of the anchors re-sorted inside every tie run so that the
    anchor tie-break reproduces the sequence.  The other anchors hold a far-off
    box with score LOW; the classes other than cls[p] hold LOW too."""
    n = len(scores)
    scores = np.asarray(scores, F32)
    assert n <= N and (scores[1:] <= scores[:-1]).all()
    if anchors is None:
        anchors = np.random.default_rng(seed).permutation(N)[:n]
        start = 0
        for p in range(1, n + 1):
            if p == n or scores[p] != scores[start]:
                anchors[start:p] = np.sort(anchors[start:p])
                start = p
    img = np.empty((4 + nc, N), F32)
    img[0], img[1], img[2], img[3] = 5000.0, 5000.0, 8.0, 8.0
    img[4:] = LOW
    if n:
        img[:4, anchors] = np.asarray(boxes, F32).T
        c = np.zeros(n, np.int64) if cls is None else np.asarray(cls, np.int64)
        img[4 + c, anchors] = scores
    return img


def kwargs(conf=CONF, iou=IOU, max_det=300, agnostic=False, max_nms=30000):
    return {"conf_thres": conf, "iou_thres": iou, "max_det": max_det, "agnostic": agnostic, "max_nms": max_nms}


def oracle(pred, kw):
    with np.errstate(invalid="ignore"):
        return NO.non_max_suppression(pred, **kw)


# ---------------------------------------------------------------- kept boxes beyond the LDS cache
def kept_beyond_lds(N=4096):
    """B=2, nc=1.  Image 0, in sorted order: 1700 disjoint lattice boxes, where
    cells 10..46 and 1100..1199 are each followed at once by a near-duplicate
    (suppressed inside its chunk; the first 37 shift the kept count off the
    chunk grid, so K passes 1024 in the middle of a chunk), then 300
    near-duplicates of cells 1030..1329 and 50 of cells 0..49: whole chunks
    whose only suppressors are kept boxes of earlier chunks, 1030.. beyond the
    LDS cache (workspace reads), 0..49 inside it.  1700 kept < max_det = 2000.
    Image 1: 1500 lattice cells, the 300 + 50 later duplicates, then cells
    1500..2099: max_det is reached in the middle of a chunk, after the
    workspace has been read."""
    follow = set(range(10, 47)) | set(range(1100, 1200))
    late = np.concatenate([near_dup(np.arange(1030, 1330)), near_dup(np.arange(0, 50))])

    def with_followers(cells):
        rows = []
        for c in cells:
            rows.append(lattice([c]))
            if c in follow:
                rows.append(near_dup([c]))
        return np.concatenate(rows)

    seq0 = np.concatenate([with_followers(range(1700)), late])
    seq1 = np.concatenate([with_followers(range(1500)), late, lattice(np.arange(1500, 2100))])
    pred = np.stack([place(seq0, seq_scores(len(seq0)), N, seed=21),
                     place(seq1, seq_scores(len(seq1)), N, seed=22)])
    return pred, kwargs(max_det=2000)


# ---------------------------------------------------------------- LDS / global sort boundary
def _grouped(n, seed):
    """n boxes in a seeded random order: concentric groups of four (16, 15, 14
    and 13 pixels wide: every pair inside a group overlaps above 0.45) on
    disjoint lattice cells, so what survives at any place of the sorted order
    depends on the order of the four - a misplaced key anywhere shows.  The
    last 64 of the order are cells of their own: kept, down to the last key."""
    rng = np.random.default_rng(seed)
    m = n - 64
    cells = np.arange(m) // 4
    size = np.asarray([16.0, 15.0, 14.0, 13.0], F32)[np.arange(m) % 4]
    boxes = lattice(cells, cols=128)
    boxes[:, 2] = boxes[:, 3] = size
    tail = lattice(cells[-1] + 1 + np.arange(64), cols=128)
    return np.concatenate([boxes[rng.permutation(m)], tail])


def keys_boundary(N=LDS_KEYS + 1):
    """B=2, nc=1, N=8193.  Image 0 (`keys_8192`): exactly NMS_LDS_KEYS
    candidates - the LDS sort with np2 == n, no ~0 padding - and one anchor
    below conf, so n != N.  Image 1 (`keys_8193`): one more, the first sort in
    the global key array, padded to 16384.  max_det = 3000 keeps every
    survivor (about n / 4) in the result, down to the tail of the order."""
    a = _grouped(LDS_KEYS, 31)
    b = _grouped(LDS_KEYS + 1, 32)
    pred = np.stack([place(a, seq_scores(len(a)), N, seed=33), place(b, seq_scores(len(b)), N, seed=34)])
    return pred, kwargs(max_det=3000)


# ---------------------------------------------------------------- chunk and word edges
CHUNK_WORD_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
CHUNK_WORD_DUPS = (((63, 64), (127, 128), (255, 256)), ((191, 192), (256, 257), (319, 320)))


def chunk_words_counts(N=513):
    """One image per n in CHUNK_WORD_COUNTS: n disjoint candidates, the other
    anchors below conf.  Every 64-bit word and 256-chunk boundary is the last
    candidate of some image."""
    pred = np.stack([place(lattice(np.arange(n)), seq_scores(n), N, seed=40 + i)
                     for i, n in enumerate(CHUNK_WORD_COUNTS)])
    return pred, kwargs(max_det=600)


def chunk_words_dups(N=513):
    """513 candidates per image, disjoint but for the pairs of sorted
    positions in CHUNK_WORD_DUPS (the later one a near-duplicate of the
    earlier): suppression across a word edge (63|64, 127|128, 191|192), across
    a chunk edge (255|256: through the kept boxes) and at the first two
    columns of a chunk (256, 257)."""
    imgs = []
    for i, pairs in enumerate(CHUNK_WORD_DUPS):
        seq = lattice(np.arange(N))
        for p, q in pairs:
            seq[q] = near_dup([p])[0]
        imgs.append(place(seq, seq_scores(N), N, seed=50 + i))
    return np.stack(imgs), kwargs(max_det=600)


# ---------------------------------------------------------------- greedy chains
def _chain(cell):
    """A, B, C: 16 x 16 boxes stepping 4 pixels: IoU(A,B) = IoU(B,C) = 12/20,
    IoU(A,C) = 8/24 <= 0.45.  Greedy keeps A and C."""
    a = lattice([cell], cols=16)[0]          # cols = 16: chains sit 4 cells apart, clear of each other
    return [a + F32([4 * k, 0, 0, 0]) for k in range(3)]


CHAIN_IN_CHUNK = ((10, 11, 12), (62, 63, 64), (100, 130, 200))
CHAIN_CROSS_CHUNK = ((100, 300, 301), (255, 256, 257), (5, 260, 520), (250, 500, 559))


def _chains(triples, n, N, seed):
    used = {p for t in triples for p in t}
    seq = np.empty((n, 4), F32)
    free = iter(range(64, 64 + n))            # lattice rows 4.. (cols = 16): below the chains' rows 0..3
    for p in range(n):
        if p not in used:
            seq[p] = lattice([next(free)], cols=16)[0]
    for k, t in enumerate(triples):
        for p, box in zip(t, _chain(4 * k)):
            seq[p] = box
    return place(seq, seq_scores(n), N, seed=seed)[None], kwargs()


def chain_in_chunk():
    """560 candidates in N = 600; A, B, C of every triple of CHAIN_IN_CHUNK at
    those sorted positions of chunk 0 (one straddles the 63|64 word edge): the
    resolver must not OR in the matrix row of the suppressed B."""
    return _chains(CHAIN_IN_CHUNK, 560, 600, 60)


def chain_cross_chunk():
    """As above with B (and C) in a later chunk than A: B dies through `csup`
    (a kept box of an earlier chunk), and its row must still stay out."""
    return _chains(CHAIN_CROSS_CHUNK, 560, 600, 61)


# ---------------------------------------------------------------- IoU exactly at the threshold
IOU_AT_THRESHOLD = {
    # thr: (width, step) of two 8-pixel-high boxes: inter / union = (w - s) / (w + s)
    0.6: (32.0, 8.0),       # 24/40 = 3/5 : fp32(3/5) > 0.6 in double -> suppressed
    0.5: (24.0, 8.0),       # 16/32 = 1/2 : equal -> strict '>' keeps it
    0.7: (136.0, 24.0),     # 112/160 = 7/10 : fp32(7/10) < 0.7 in double -> kept
}


def iou_at_threshold(thr, classes=(0, 0), nc=1, agnostic=False):
    """N = 2: box A (score 0.9) and box B (0.8) whose fp32 IoU is the fp32
    rounding of `thr` itself.  classes: the class of A and of B."""
    w, s = IOU_AT_THRESHOLD[thr]
    boxes = F32([[w / 2 + 8, 12, w, 8], [w / 2 + 8 + s, 12, w, 8]])
    img = place(boxes, F32([0.9, 0.8]), 2, nc=nc, cls=classes, anchors=np.asarray([1, 0]))
    return img[None], kwargs(iou=thr, agnostic=agnostic)


# ---------------------------------------------------------------- max_nms / max_det
MAX_NMS_EDGES = (1, 255, 256, 257)
MAX_NMS_TIE_CUT = 300


def max_nms_edges(max_nms):
    """nc=2, N=1000, every anchor a candidate, scores tied in runs of 7 (so
    every cut of MAX_NMS_EDGES and MAX_NMS_TIE_CUT falls inside a tie run and
    is decided by the anchor index).  Cells 0..799 once, cells 600..799 a
    second time as near-duplicates of the same class, in a seeded order; the
    box at sorted position MAX_NMS_TIE_CUT is cell 0, which nothing overlaps."""
    rng = np.random.default_rng(70)
    cells = np.concatenate([np.arange(1, 800), np.arange(600, 800)])
    boxes = np.concatenate([lattice(np.arange(1, 800)), near_dup(np.arange(600, 800))])
    perm = rng.permutation(len(cells))
    cells, boxes = cells[perm], boxes[perm]
    cells = np.insert(cells, MAX_NMS_TIE_CUT, 0)
    boxes = np.insert(boxes, MAX_NMS_TIE_CUT, lattice([0]), axis=0)
    img = place(boxes, seq_scores(1000, run=7), 1000, nc=2, cls=cells % 2, seed=71)
    return img[None], kwargs(max_det=1000, max_nms=max_nms)


def max_det_edges(max_det):
    """nc=1, N=400: 300 disjoint candidates.  max_det = 256 stops exactly at
    the end of chunk 0, 257 one box into chunk 1, 1 at the first box."""
    return place(lattice(np.arange(300)), seq_scores(300), 400, seed=80)[None], kwargs(max_det=max_det)


# ---------------------------------------------------------------- scan kernel: class loop
SCAN_NCS = (1, 2, 8, 9, 10, 16, 17)
ARGMAX_TIE_PAIRS = ((0, 8), (8, 9), (1, 16), (7, 8))


def argmax_tie_pairs(nc):
    """The (lower, higher) class pairs that tie for the maximum at nc classes:
    the listed ones that fit, and (0, nc - 1)."""
    pairs = [p for p in ARGMAX_TIE_PAIRS if p[1] < nc]
    if nc >= 2 and (0, nc - 1) not in pairs:
        pairs.append((0, nc - 1))
    return pairs


def tie_box(t):
    """Tie anchor t's box: far from everything else, so it is always kept."""
    return F32([3000 + 20 * t, 3000, 16, 16])


def scan_class_loop(nc, N=257):
    """Anchor t < len(pairs) holds the maximum 0.95 at both classes of pair t
    (first argmax = the lower) in a far-off box; the other anchors hold
    clustered boxes, class scores below 0.2 and - six in seven - one class
    (cycling over all nc) raised above conf."""
    rng = np.random.default_rng(90 + nc)
    img = np.empty((4 + nc, N), F32)
    centres = rng.integers(0, 40, (6, 2)) * 16
    pick = rng.integers(0, 6, N)
    img[0] = centres[pick, 0] + rng.integers(-6, 7, N) * 2 + 100
    img[1] = centres[pick, 1] + rng.integers(-6, 7, N) * 2 + 100
    img[2:4] = rng.integers(8, 40, (2, N)) * 2
    img[4:] = (rng.integers(0, 50, (nc, N)) / 256).astype(F32)
    a = np.arange(N)
    hot = a % 7 != 6
    img[4 + (a % nc)[hot], a[hot]] = (F32(0.3) + rng.integers(0, 150, N).astype(F32) / F32(256))[hot]
    for t, (lo, hi) in enumerate(argmax_tie_pairs(nc)):
        img[:4, t] = tie_box(t)
        img[4:, t] = rng.integers(0, 50, nc) / 256
        img[4 + lo, t] = img[4 + hi, t] = 0.95
    return img[None], kwargs()


# ---------------------------------------------------------------- scan kernel: wave compaction
SCAN_WAVE_NS = (1, 63, 64, 65, 255, 257)


def scan_waves(N):
    """nc=3, six images of disjoint boxes whose candidates are: every anchor;
    anchor 0 alone (lane 0); anchor min(63, N-1) alone (lane 63); the last
    anchor alone; the anchors of waves 0 and 3 only; every other anchor."""
    a = np.arange(N)
    masks = [np.ones(N, bool), a == 0, a == min(63, N - 1), a == N - 1, (a < 64) | (a // 64 == 3), a % 2 == 1]
    imgs = []
    rng = np.random.default_rng(100 + N)
    for m in masks:
        img = np.empty((7, N), F32)
        img[:4] = lattice(a).T
        img[4:] = LOW
        score = rng.permutation(seq_scores(N))
        img[4 + a % 3, a] = np.where(m, score, LOW)
        imgs.append(img)
    return np.stack(imgs), kwargs()


# ---------------------------------------------------------------- batch strides
def _dense(nc, N, seed):
    """Clustered random boxes, every anchor a candidate, scores in sixteenths
    (ties) - real suppression work."""
    rng = np.random.default_rng(seed)
    img = np.empty((4 + nc, N), F32)
    centres = rng.integers(0, 80, (4, 2)) * 8
    pick = rng.integers(0, 4, N)
    img[0] = centres[pick, 0] + rng.integers(-8, 9, N)
    img[1] = centres[pick, 1] + rng.integers(-8, 9, N)
    img[2:4] = rng.integers(40, 100, (2, N))
    img[4:] = (rng.integers(5, 16, (nc, N)) / 16).astype(F32)
    return img


def batch_mix(B=33, nc=4, N=700):
    """Image b: b % 4 == 0 empty, 1 one candidate, 2 dense clusters, 3 more
    disjoint boxes than max_det = 100 - neighbours of different kinds, so a
    wrong per-image stride of the keys, classes, kept boxes or counts shows."""
    imgs = []
    for b in range(B):
        kind = b % 4
        if kind == 0:
            img = place(np.empty((0, 4), F32), np.empty(0, F32), N, nc=nc)
        elif kind == 1:
            img = place(lattice([b]), F32([0.5 + b / 128]), N, nc=nc, cls=[b % nc], seed=110 + b)
        elif kind == 2:
            img = _dense(nc, N, 110 + b)
        else:
            n = 400 + b
            img = place(lattice(np.arange(n)), seq_scores(n), N, nc=nc, cls=np.arange(n) % nc, seed=110 + b)
        imgs.append(img)
    return np.stack(imgs), kwargs(max_det=100)


# ---------------------------------------------------------------- plan reuse / graph replay
def reuse_sequence():
    """Four (2, 5, 8193) inputs for one plan (max_det = 3000), in this order:
    the sort-boundary pair, ten candidates, a dense image with kept boxes
    beyond the LDS cache, nothing - each must leave no trace for the next."""
    N = LDS_KEYS + 1
    kw = kwargs(max_det=3000)
    few = np.stack([place(lattice(np.arange(10)), seq_scores(10), N, seed=120),
                    place(near_dup(np.arange(10)), seq_scores(10), N, seed=121)])
    empty = np.stack([place(np.empty((0, 4), F32), np.empty(0, F32), N)] * 2)
    return [keys_boundary(N)[0], few, kept_beyond_lds(N)[0], empty], kw


def graph_sequence():
    """Three (1, 5, 8193) inputs with 0, 300 and 8193 candidates for one
    captured launch sequence."""
    N = LDS_KEYS + 1
    none = place(np.empty((0, 4), F32), np.empty(0, F32), N)[None]
    some = place(lattice(np.arange(300)), seq_scores(300), N, seed=130)[None]
    return [none, some, keys_boundary(N)[0][1:]], kwargs(max_det=3000)


# ---------------------------------------------------------------- non-finite values
NAN_NC = 10      # classes 1..8: the unrolled group of the scan's class loop, 9: its remainder
# (class 0 score, {class: score}) of each NaN anchor kind; every finite score is above conf
NAN_FIRST = ((np.nan, {2: 0.8}), (np.nan, {9: 0.8}), (np.nan, {c: np.nan for c in range(1, NAN_NC)}))
NAN_LATER = ((0.8, {3: np.nan}), (0.8, {9: np.nan}), (0.8, {5: np.nan, 7: 0.9}), (0.8, {1: 0.9, 8: np.nan}),
             (0.8, {9: np.nan, 4: 0.85}))


def nan_scores(N=130):
    """nc=10, disjoint boxes.  Anchor a is of kind a % 16: kinds 0..2 carry a
    NaN at class 0 (NAN_FIRST), kinds 3..7 a finite class 0 and a NaN later
    (NAN_LATER: in the unrolled group, in the remainder, before and after a
    larger finite score), the others are plain candidates.  `amax` drops every
    anchor of kinds 0..7."""
    kinds = NAN_FIRST + NAN_LATER
    img = np.empty((4 + NAN_NC, N), F32)
    img[:4] = lattice(np.arange(N)).T
    img[4:] = LOW
    score = np.random.default_rng(140).permutation(seq_scores(N))
    for a in range(N):
        k = a % 16
        if k < len(kinds):
            img[4, a] = kinds[k][0]
            for c, v in kinds[k][1].items():
                img[4 + c, a] = v
        else:
            img[4 + a % NAN_NC, a] = score[a]
    return img[None], kwargs()


def nan_kind(a):
    return a % 16


def inf_score(N=70):
    """nc=2: +inf class scores (two of them tie and overlap) among finite ones."""
    seq = lattice(np.arange(N))
    seq[1] = near_dup([0])[0]
    seq[5] = near_dup([4])[0]
    s = seq_scores(N)
    s[:3] = np.inf
    return place(seq, s, N, nc=2, cls=np.arange(N) // 2 % 2, seed=150)[None], kwargs()


def nonfinite_boxes(N=40):
    """nc=1: candidates whose box has a NaN x, a NaN w, an inf w or an inf x
    among finite boxes that overlap where those would lie.  Every IoU with
    such a box is NaN or 0: it is kept and suppresses nothing."""
    seq = lattice(np.arange(N))
    for p in (3, 9, 17, 25):
        seq[p + 1] = near_dup([p])[0]          # the next box would be suppressed by a finite box here
    seq[3, 0] = np.nan
    seq[9, 2] = np.nan
    seq[17, 2] = np.inf
    seq[25, 0] = np.inf
    seq[30] = seq[17]                           # a second inf-wide box on the same row
    return place(seq, seq_scores(N), N, seed=160)[None], kwargs()


def signed_zeros(N=64):
    """nc=1, conf_thres = -1: scores +0.0 and -0.0 at interleaved anchors
    (and +-0.5 around them).  Zeros of either sign tie: anchor order.  Boxes
    repeat every 7 anchors (both signs in every stack of concentric boxes), so
    which zero comes first decides what is kept."""
    img = np.empty((5, N), F32)
    a = np.arange(N)
    img[:4] = lattice(a % 7).T
    img[2] = 16 - (a // 7) % 3
    img[4] = np.where(a % 2 == 0, F32(0.0), F32(-0.0))
    img[4, a % 16 == 5] = 0.5
    img[4, a % 16 == 10] = -0.5
    return img[None], kwargs(conf=-1.0)
