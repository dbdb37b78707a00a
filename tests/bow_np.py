"""numpy restatement of BoW generation as BoW/test_bow.cpp runs it (ORB_SLAM2::ORBVocabulary = DBoW2 TemplatedVocabulary<FORB>):
the text loader's rules (TemplatedVocabulary.h:1338-1424), the descent (:1218-1260, FORB.cpp:81-97), the BowVector accumulation and
normalisation in the reference's order (:1127-1193, BowVector.cpp:30-69, ScoringObject.h:74-90) and the output writer (test_bow.cpp:146-163).
Python floats are IEEE doubles, and every sum here is the reference's own sequence of additions."""
import math

import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
TF_IDF, TF, IDF, BINARY = range(4)


class Vocab:
    """Node arrays with the root at index 0 (parent [n], is_leaf [n], desc [n, 32], weight [n])."""

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, desc, weight):
        self.k, self.L, self.scoring, self.weighting = int(k), int(L), int(scoring), int(weighting)
        self.parent = np.asarray(parent, np.int64)
        self.is_leaf = np.asarray(is_leaf) > 0
        self.is_leaf[0] = False
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.asarray(weight, np.float64)
        n = len(self.parent)
        self.word = np.zeros(n, np.int64)                    # Node(): word_id(0); leaves numbered in node order
        self.word[np.flatnonzero(self.is_leaf)] = np.arange(int(self.is_leaf.sum()))
        self.n_words = int(self.is_leaf.sum())
        cnt = np.bincount(self.parent[1:], minlength=n) if n > 1 else np.zeros(n, np.int64)
        self.cstart = np.concatenate([[0], np.cumsum(cnt)])
        self.kids = np.argsort(self.parent[1:], kind="stable") + 1 if n > 1 else np.zeros(0, np.int64)   # children in id order
        self.ccount = cnt


def parse_text(text: str) -> Vocab:
    """loadFromTextFile's rules; ValueError where the library returns PR_EINVAL (header limits, < 35 tokens, non-numbers, a parent that
    is not an earlier node).  Empty lines are skipped."""
    lines = text.split("\n")
    h = lines[0].split()
    if len(h) < 4:
        raise ValueError("line 1: header")
    k, L, sc, wt = (int(x) for x in h[:4])
    if k < 0 or k > 20 or L < 1 or L > 10 or sc < 0 or sc > 5 or wt < 0 or wt > 3:
        raise ValueError("line 1: header limits")
    parent, leaf, desc, weight = [-1], [0], [[0] * 32], [0.0]
    for no, line in enumerate(lines[1:], start=2):
        t = line.split()
        if not t:
            continue
        if len(t) < 35:
            raise ValueError(f"line {no}: {len(t)} tokens")
        p = int(t[0])
        if p < 0 or p >= len(parent):
            raise ValueError(f"line {no}: parent {p}")
        parent.append(p)
        leaf.append(int(t[1]) > 0)
        desc.append([int(x) % 256 for x in t[2:34]])
        weight.append(float(t[34]))
    return Vocab(k, L, sc, wt, parent, leaf, desc, weight)


def to_text(v: Vocab, fmt=repr) -> str:
    """ORBvoc-style text of v (saveToTextFile's layout), weights written with `fmt`."""
    out = [f"{v.k} {v.L} {v.scoring} {v.weighting}"]
    for i in range(1, len(v.parent)):
        out.append(f"{v.parent[i]} {int(v.is_leaf[i])} " + " ".join(str(int(b)) for b in v.desc[i]) + f" {fmt(float(v.weight[i]))}")
    return "\n".join(out) + "\n"


def descend(v: Vocab, desc) -> np.ndarray:
    """The childless node each descriptor's descent ends on: children[0] first, a later child only if strictly closer."""
    d = np.asarray(desc, np.uint8).reshape(-1, 32)
    cur = np.zeros(len(d), np.int64)
    while True:
        act = np.flatnonzero(v.ccount[cur] > 0)
        if len(act) == 0:
            return cur
        c = cur[act]
        cnt = v.ccount[c]
        best_d = np.full(len(act), 1 << 30)
        best = np.zeros(len(act), np.int64)
        for j in range(int(cnt.max())):
            m = j < cnt
            cid = v.kids[np.where(m, v.cstart[c] + j, 0)]
            dist = POPCOUNT[d[act] ^ v.desc[cid]].sum(axis=1)
            upd = m & (dist < best_d)
            best_d = np.where(upd, dist, best_d)
            best = np.where(upd, cid, best)
        cur[act] = best


def transform(v: Vocab, desc):
    """BowVector of one image: (word ids ascending, values) as Python lists."""
    if v.n_words == 0:
        return [], []
    nodes = descend(v, desc)
    bv = {}
    tf = v.weighting in (TF_IDF, TF)
    for nd in nodes:
        w = float(v.weight[nd])
        wid = int(v.word[nd])
        if w > 0:
            if tf:
                bv[wid] = bv[wid] + w if wid in bv else w    # addWeight
            elif wid not in bv:
                bv[wid] = w                                   # addIfNotExist
    ids = sorted(bv)
    vals = [bv[i] for i in ids]
    must = v.scoring != DOT_PRODUCT
    if tf and ids and not must:
        nd = float(len(ids))
        vals = [x / nd for x in vals]
    if must:
        norm = 0.0
        if v.scoring == L2_NORM:
            for x in vals:
                norm += x * x
            norm = math.sqrt(norm)
        else:
            for x in vals:
                norm += abs(x)
        if norm > 0.0:
            vals = [x / norm for x in vals]
    return ids, vals


def rows(v: Vocab, images, cols: int) -> np.ndarray:
    """[2N, cols] ids / values rows padded with -1 (pr_bow_distance's layout); images: a list of uint8 [n, 32]."""
    out = -np.ones((2 * len(images), cols))
    for i, d in enumerate(images):
        ids, vals = transform(v, d)
        n = min(len(ids), cols)
        out[2 * i, :n] = ids[:n]
        out[2 * i + 1, :n] = vals[:n]
    return out


def write_history(bvs) -> str:
    """test_bow.cpp:146-163: ids then values, `x << " "` each at default ostream precision, "-1 " up to 4000 entries, std::endl."""
    out = []
    for ids, vals in bvs:
        pad = "-1 " * max(0, 4000 - len(ids))
        out.append("".join(f"{i} " for i in ids) + pad + "\n")
        out.append("".join("%g " % x for x in vals) + pad + "\n")
    return "".join(out)
