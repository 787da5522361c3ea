"""The small random index the width / shape tests of the inner-product, polysemous and IVFFlat scans share (TEST
INFRASTRUCTURE ONLY): fixed list lengths on both sides of every boundary of the kernels' walk (a wave takes 64 codes of
every 256), probes with holes, negative ids.  Seeded: the same arguments give the same arrays.

  LENGTHS   0 (skipped), 1, 63 / 64 / 65 (the wave boundary), 256 / 257 (the trip boundary), 1600 (seven trips, the last one
            partial, the prefetch of the last trip clamped; at a pass rate above a third more than 512 passers, so the
            polysemous ring of 128 slots per wave wraps), and four ordinary lists.  2600 codes.
  keys      every query: the first nprobe of a random permutation of the occupied lists, about 15 % of them replaced by -1.
            Five rows are then set by hand so that the conditions hold by construction and not by luck: query 0 starts with
            the long list, query 1 with a hole and then the long list (so a max_codes cut still lets it through), query 2
            walks the seven boundary lengths in order, query 3 sees 64 codes in all (a partly padded row from k = 65 on),
            query 4 has no probe at all (a row of padding).
  ids       a random permutation times 5 minus 7: negative ids occur, no id is its own position.
"""
import numpy as np

LENGTHS = (257, 0, 64, 1600, 1, 63, 100, 65, 256, 37, 130, 27)
REQUIRED = (0, 1, 63, 64, 65, 256, 257)
SHORT_LENGTHS = (257, 0, 64, 700, 1, 63, 10, 65, 256, 5, 13, 7)      # the same boundaries with fewer codes (wide rows)
LONG = 700                                                           # "the long list": at least this many codes


def layout(seed=0, nlist=12, lengths=LENGTHS, nq=24, nprobe=7, holes=0.15):
    """dict: nlist, lens [nlist], list_offsets [nlist + 1], ids [ntotal], keys [nq][nprobe], nq, nprobe.  nlist > len(lengths)
    leaves the other lists empty and unprobed (a multi-index quantizer has 4^n lists)."""
    rng = np.random.default_rng(9000 + seed)
    nocc = len(lengths)
    assert nlist >= nocc and nprobe <= nocc and nq >= 5
    where = np.sort(rng.permutation(nlist)[:nocc])             # list numbers that carry the given lengths, in order
    lens = np.zeros(nlist, np.int64)
    lens[where] = lengths
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    ntotal = int(off[-1])
    ids = rng.permutation(ntotal).astype(np.int64) * 5 - 7
    keys = np.stack([where[rng.permutation(nocc)[:nprobe]] for _ in range(nq)]).astype(np.int64)
    keys[rng.random(keys.shape) < holes] = -1
    by_len = {int(n): int(w) for w, n in zip(where, lengths)}
    longest = int(where[int(np.argmax(lengths))])

    def put_first(row, first):
        rest = [int(k) for k in keys[row] if k != longest]
        keys[row] = (list(first) + rest)[:nprobe]

    put_first(0, [longest])
    put_first(1, [-1, longest])
    if nprobe >= len(REQUIRED) and all(n in by_len for n in REQUIRED):
        keys[2, :len(REQUIRED)] = [by_len[n] for n in REQUIRED]
        keys[3] = -1
        keys[3, [0, 2, 3]] = [by_len[1], by_len[0], by_len[63]]
    keys[4] = -1
    return dict(nlist=nlist, lens=lens, list_offsets=off, ids=ids, keys=keys, nq=nq, nprobe=nprobe, ntotal=ntotal)


def probed_lengths(lay):
    """lengths of the lists some query probes"""
    k = lay["keys"]
    return set(int(n) for n in lay["lens"][np.unique(k[k >= 0])])


def check_layout(lay, long=LONG):
    """the conditions the tests rely on: every boundary length present and probed, a long list probed, holes, negative ids"""
    lens, seen = lay["lens"], probed_lengths(lay)
    for n in REQUIRED:
        assert (lens == n).any(), "no list of %d codes" % n
        assert n in seen, "no query probes the list of %d codes" % n
    assert lens.max() >= long and int(lens.max()) in seen, "no probed list of %d codes or more" % long
    assert (lay["keys"] < 0).any() and (lay["ids"] < 0).any()
    for row in lay["keys"]:
        live = row[row >= 0]
        assert np.unique(live).size == live.size, "a list probed twice by one query"


def pq_parts(lay, M, dsub, nbits, seed=0):
    """general floats and random codes for an IVFPQ index over the layout: coarse [nlist][d], pq [M][ksub][dsub],
    codes [ntotal][M], xq [nq][d], coarse_dis [nq][nprobe] (arbitrary positive floats: table types 1 and 2 add them)"""
    rng = np.random.default_rng(9100 + 1000 * seed + 64 * M + 8 * dsub + nbits)
    d, ksub = M * dsub, 1 << nbits
    return dict(d=d, M=M, nbits=nbits, ksub=ksub, dsub=dsub,
                coarse=rng.standard_normal((lay["nlist"], d)).astype(np.float32),
                pq=(0.5 * rng.standard_normal((M, ksub, dsub))).astype(np.float32),
                codes=rng.integers(0, ksub, (lay["ntotal"], M), dtype=np.uint8),
                xq=rng.standard_normal((lay["nq"], d)).astype(np.float32),
                coarse_dis=(rng.random((lay["nq"], lay["nprobe"])) * 9 + 1).astype(np.float32))


def flat_parts(lay, d, seed=0):
    """general floats for an IVFFlat index over the layout: coarse [nlist][d], vecs [ntotal][d], xq [nq][d]"""
    rng = np.random.default_rng(9200 + 1000 * seed + d)
    return dict(d=d, coarse=rng.standard_normal((lay["nlist"], d)).astype(np.float32),
                vecs=rng.standard_normal((lay["ntotal"], d)).astype(np.float32),
                xq=rng.standard_normal((lay["nq"], d)).astype(np.float32))


def input_order(lay, seed=0):
    """a random interleaving of the lists that keeps the order inside every list: (rows [ntotal] into the list-contiguous
    arrays, assign [ntotal]).  Adding rows in this order with this assignment rebuilds the layout's lists."""
    rng = np.random.default_rng(9300 + seed)
    u = rng.random(lay["ntotal"])
    off = lay["list_offsets"]
    for i in range(lay["nlist"]):
        u[off[i]:off[i + 1]].sort()
    rows = np.argsort(u, kind="stable")
    assign = np.repeat(np.arange(lay["nlist"], dtype=np.int64), lay["lens"])[rows]
    return rows, assign
