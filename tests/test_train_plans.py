"""CPU: the launch plans of the three training kernels are pure host functions (csrc/pq_train_plan.h: plan_pq_assign,
csrc/kmeans_plan.h: plan_kmeans_update, csrc/moments_plan.h: plan_moments).  tests/cpp/train_plan_dump.cpp -- host compiler only, over
a three-name stand-in for the HIP header -- prints the plan of every shape the GPU shape tests run (test_gpu_pq_train_shapes.py,
test_gpu_kmeans_shapes.py, test_gpu_moments_shapes.py); the expected values are written by hand from the rules of the headers:

  pq    dsub = d / M, cols = ksub rounded up to 32, kq = ceil(dsub / 8), stride = 4 kq (kq odd) or 4 kq + 4
        lds(g) = g (2 cols stride + cols) 4 + 4 g (64 stride + 32) 4
        loop route: n < 20 with dsub % 4 == 0, or lds(1) > 160 KiB; otherwise batched with
        group = min(ceil(32 / dsub), M), halved (rounding up) while lds(group) > 160 KiB; ngroups = ceil(M / group)
        vec = d % 4 == 0 and dsub % 4 == 0; grid.x = min(ceil(256 min(160 KiB / lds, 2) / ngroups), ceil(n / 128)), grid.y = ngroups
  km    key_row_bits = bits(max(n - 1, 1)), key_bits = that + bits(k - 1)
        d < 64: packed, grid ceil(k d / 256); else slices = ceil(d / 64), waves = min(slices, 4), grid k x ceil(slices / waves)
  mom   tiles = ceil(d / 128) a side; pairs = tiles_x tiles_y, symmetric tiles (tiles + 1) / 2; kr = 32 unless 16 or 64 is forced
        s = forced, else min(512 / pairs, n / (4 kr)); at least 1, at most n; slice_len = ceil(n / s) rounded up to kr;
        S = ceil(n / slice_len); scratch = S pairs 65536; col_slice_len = max(ceil(n / 4096), 256) rounded up to 4
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
CSRC = os.path.join(ROOT, "vector_line_quantization_amd", "csrc")
LDS_LIMIT = 160 * 1024
WHY_LDS = "one slice's codebook does not fit 160 KB of LDS beside the row tile"
WHY_FEW = "fewer than 20 rows with dsub % 4 == 0: the flat search's per-pair order"

# (n, d, M, nbits): route, cols, kq, stride, group, ngroups, vec, lds, grid
PQ_SHAPES = [
    # the assignment cases of test_gpu_pq_train_shapes.py
    ((300, 48, 6, 4), ("batched", 32, 1, 4, 4, 2, 1, 23040, "3x2")),            # dsub 8: groups of 4 and 2
    ((200, 48, 8, 3), ("batched", 32, 1, 4, 6, 2, 0, 34560, "2x2")),            # dsub 6: groups of 6 and 2, scalar loads
    ((300, 32, 32, 8), ("batched", 256, 1, 4, 8, 4, 0, 110592, "3x4")),         # dsub 1: 32 -> 16 -> 8 (442368, 221184, 110592 bytes)
    ((300, 32, 16, 8), ("batched", 256, 1, 4, 8, 2, 0, 110592, "3x2")),         # dsub 2: 16 -> 8
    ((300, 32, 4, 5), ("batched", 32, 1, 4, 4, 1, 1, 23040, "3x1")),
    ((300, 32, 4, 6), ("batched", 64, 1, 4, 4, 1, 1, 27648, "3x1")),
    ((300, 32, 4, 7), ("batched", 128, 1, 4, 4, 1, 1, 36864, "3x1")),
    ((300, 104, 1, 8), ("batched", 256, 13, 52, 1, 1, 1, 161280, "3x1")),       # the largest batched codebook
    ((300, 105, 1, 8), ("loop", 256, 14, 60, 1, 1, 0, 0, "1x1")),               # 185856 bytes: does not fit
    ((300, 224, 2, 8), ("loop", 256, 14, 60, 1, 2, 0, 0, "1x1")),
    ((2049, 2048, 64, 2), ("batched", 32, 4, 20, 1, 64, 1, 26240, "8x64")),     # 17 row tiles under 8 walkers
    ((300, 32, 4, 4), ("batched", 32, 1, 4, 4, 1, 1, 23040, "3x1")),            # the value cases
    # the training cases
    ((600, 128, 2, 4), ("batched", 32, 8, 36, 1, 2, 1, 46720, "5x2")),
    ((300, 192, 2, 3), ("batched", 32, 12, 52, 1, 2, 1, 67200, "3x2")),
    ((200, 496, 2, 3), ("batched", 32, 31, 124, 1, 2, 1, 159360, "2x2")),       # the widest batched dsub at cols 32
    ((200, 512, 2, 3), ("loop", 32, 32, 132, 1, 2, 0, 0, "1x1")),               # (dsub 249 .. 256: 169600 bytes)
    ((500, 40, 4, 4), ("batched", 32, 2, 12, 4, 1, 0, 64000, "4x1")),
    ((400, 48, 6, 4), ("batched", 32, 1, 4, 4, 2, 1, 23040, "4x2")),
    ((600, 105, 1, 8), ("loop", 256, 14, 60, 1, 1, 0, 0, "1x1")),
    ((33000, 8, 2, 7), ("batched", 128, 1, 4, 2, 1, 1, 18432, "258x1")),        # test_gpu_kmeans_shapes.py: the batched objective
    ((16, 8, 2, 3), ("loop", 32, 1, 4, 1, 2, 0, 0, "1x1")),                     # the other reason for the loop route
]
PQ_UNSUPPORTED = [(0, 8, 2, 3), (10, 8, 3, 3), (10, 8, 2, 0), (10, 8, 2, 9), (1 << 30, 8, 2, 3)]

# (n, k, d): packed, waves, slices, key_row_bits, key_bits, grid
KM_SHAPES = [
    ((2345, 12, 5), (1, 4, 0, 12, 16, "1x1")),
    ((2345, 12, 63), (1, 4, 0, 12, 16, "3x1")),
    ((2345, 12, 64), (0, 1, 1, 12, 16, "12x1")),
    ((2345, 12, 130), (0, 3, 3, 12, 16, "12x1")),
    ((700, 9, 63), (1, 4, 0, 10, 14, "3x1")),
    ((700, 9, 256), (0, 4, 4, 10, 14, "9x1")),
    ((700, 9, 257), (0, 4, 5, 10, 14, "9x2")),                  # a second workgroup per centroid, one live lane in it
    ((700, 9, 300), (0, 4, 5, 10, 14, "9x2")),
    ((1024, 256, 4), (1, 4, 0, 10, 18, "4x1")),
    ((1025, 257, 4), (1, 4, 0, 11, 20, "5x1")),
    ((1000, 1, 8), (1, 4, 0, 10, 10, "1x1")),                   # one cluster: no centroid bits in the key
    ((2, 2, 3), (1, 4, 0, 1, 2, "1x1")),
    ((1, 1, 1), (1, 4, 0, 1, 1, "1x1")),
    ((33000, 130, 4), (1, 4, 0, 16, 24, "3x1")),
    # the updates inside batched PQ training: (n M, M ksub, dsub)
    ((1200, 32, 64), (0, 1, 1, 11, 16, "32x1")),
    ((600, 16, 96), (0, 2, 2, 10, 14, "16x1")),
    ((400, 16, 248), (0, 4, 4, 9, 13, "16x1")),
    ((2000, 64, 10), (1, 4, 0, 11, 17, "3x1")),
    ((2400, 96, 8), (1, 4, 0, 12, 19, "3x1")),
    ((66000, 256, 4), (1, 4, 0, 17, 25, "4x1")),
]

# (n, dx, dy, symmetric, forced kr, forced slices): kr, tiles, pairs, S, slice_len, col_slices
MOM_SHAPES = [
    ((300, 100, 300, 0, 0, 0), (32, "1x3", 3, 2, 160, 2)),
    ((300, 300, 100, 0, 0, 0), (32, "3x1", 3, 2, 160, 2)),
    ((200, 129, 127, 0, 0, 0), (32, "2x1", 2, 1, 224, 1)),
    ((300, 300, 0, 1, 0, 0), (32, "3x3", 6, 2, 160, 2)),
    ((200, 129, 0, 1, 0, 0), (32, "2x2", 3, 1, 224, 1)),
    ((128, 128, 0, 1, 0, 0), (32, "1x1", 1, 1, 128, 1)),
    ((32, 7, 0, 1, 0, 0), (32, "1x1", 1, 1, 32, 1)),
    # set_split at (1000, 130, 130): S is recomputed from the rounded slice_len
    ((1000, 130, 0, 1, 16, 0), (16, "2x2", 3, 13, 80, 4)),
    ((1000, 130, 0, 1, 16, 1), (16, "2x2", 3, 1, 1008, 4)),
    ((1000, 130, 0, 1, 16, 7), (16, "2x2", 3, 7, 144, 4)),
    ((1000, 130, 0, 1, 16, 9), (16, "2x2", 3, 9, 112, 4)),
    ((1000, 130, 0, 1, 64, 0), (64, "2x2", 3, 3, 384, 4)),
    ((1000, 130, 0, 1, 64, 1), (64, "2x2", 3, 1, 1024, 4)),
    ((1000, 130, 0, 1, 64, 7), (64, "2x2", 3, 6, 192, 4)),                  # 7 asked for: 143 rows round up to 192, six slices
    ((1000, 130, 0, 1, 64, 9), (64, "2x2", 3, 8, 128, 4)),                  # 9 asked for: 112 rows round up to 128, eight slices
    ((1000, 130, 130, 0, 16, 0), (16, "2x2", 4, 13, 80, 4)),
    ((1000, 130, 130, 0, 16, 1), (16, "2x2", 4, 1, 1008, 4)),
    ((1000, 130, 130, 0, 16, 7), (16, "2x2", 4, 7, 144, 4)),
    ((1000, 130, 130, 0, 16, 9), (16, "2x2", 4, 9, 112, 4)),
    ((1000, 130, 130, 0, 64, 0), (64, "2x2", 4, 3, 384, 4)),
    ((1000, 130, 130, 0, 64, 1), (64, "2x2", 4, 1, 1024, 4)),
    ((1000, 130, 130, 0, 64, 7), (64, "2x2", 4, 6, 192, 4)),
    ((1000, 130, 130, 0, 64, 9), (64, "2x2", 4, 8, 128, 4)),
    ((100, 40, 0, 1, 32, 50), (32, "1x1", 1, 4, 32, 1)),                    # 50 slices asked for, four strips exist
    ((100, 40, 0, 1, 0, 0), (32, "1x1", 1, 1, 128, 1)),
    ((257, 64, 0, 1, 0, 0), (32, "1x1", 1, 2, 160, 2)),
    ((257, 64, 64, 0, 0, 0), (32, "1x1", 1, 2, 160, 2)),
    # host rows: the plan of a full page of 32 768 rows
    ((32768, 20, 36, 0, 0, 0), (32, "1x1", 1, 256, 128, 128)),
    ((32768, 20, 0, 1, 0, 0), (32, "1x1", 1, 256, 128, 128)),
    ((32768, 20, 0, 1, 64, 0), (64, "1x1", 1, 128, 256, 128)),
    # train_pca: 5000 rows and its subsample of 2000
    ((5000, 40, 0, 1, 0, 0), (32, "1x1", 1, 32, 160, 20)),
    ((2000, 40, 0, 1, 0, 0), (32, "1x1", 1, 13, 160, 8)),
]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("train_plan") / "train_plan_dump")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(CPP, "hip_stub"), "-I" + CSRC,
                           os.path.join(CPP, "train_plan_dump.cpp"), "-o", exe])

    def run(kind, shapes):
        text = "".join("%s %s\n" % (kind, " ".join(str(v) for v in s)) for s in shapes)
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.splitlines()
        assert len(lines) == len(shapes)
        return lines
    return run


def fields(line):
    return dict(kv.split("=", 1) for kv in line.split(": ", 1)[1].split(" why=")[0].split())


def test_pq_assign_plan_of_every_shape(dump):
    for line, ((n, d, M, nbits), (route, cols, kq, stride, group, ngroups, vec, lds, grid)) in zip(dump("pq", [s for s, _w in PQ_SHAPES]), PQ_SHAPES):
        why = "" if route == "batched" else WHY_FEW if n < 20 else WHY_LDS
        want = "pq n=%d d=%d M=%d nbits=%d: route=%s dsub=%d ksub=%d cols=%d kq=%d stride=%d group=%d ngroups=%d vec=%d lds=%d grid=%s why=%s" % (
            n, d, M, nbits, route, d // M, 1 << nbits, cols, kq, stride, group, ngroups, vec, lds, grid, why)
        assert line == want
    for line in dump("pq", PQ_UNSUPPORTED):
        assert ": unsupported (" in line, line


def test_kmeans_update_plan_of_every_shape(dump):
    for line, ((n, k, d), (packed, waves, slices, row_bits, key_bits, grid)) in zip(dump("km", [s for s, _w in KM_SHAPES]), KM_SHAPES):
        want = "km n=%d k=%d d=%d: kernel=%s packed=%d waves=%d slices=%d key_row_bits=%d key_bits=%d grid=%s" % (
            n, k, d, "kmeans_update_packed_kernel" if packed else "kmeans_update_kernel", packed, waves, slices, row_bits, key_bits, grid)
        assert line == want


def test_moments_plan_of_every_shape(dump):
    for line, ((n, dx, dy, sym, fkr, fs), (kr, tiles, pairs, S, slice_len, col_slices)) in zip(dump("mom", [s for s, _w in MOM_SHAPES]), MOM_SHAPES):
        want = "mom n=%d dx=%d dy=%d sym=%d kr=%d fs=%d: kr=%d tiles=%s pairs=%d S=%d slice_len=%d lds=%d scratch=%d col_slices=%d col_slice_len=256" % (
            n, dx, dy, sym, fkr, fs, kr, tiles, pairs, S, slice_len, 4 * kr * 128 * 4, S * pairs * 65536, col_slices)
        assert line == want


def pq_lds(g, cols, stride):
    return g * (2 * cols * stride + cols) * 4 + 4 * g * (2 * 32 * stride + 32) * 4


def test_pq_assign_plan_invariants(dump):
    shapes = [(n, dsub * M, M, nbits) for dsub in range(1, 301) for M in (1, 2, 3, 5, 8, 33, 64) for nbits in range(1, 9)
              for n in (1, 19, 20, 127, 128, 129, 100000)]
    seen = {"batched": 0, "loop": 0, "halved": 0, "ragged": 0}
    for (n, d, M, nbits), line in zip(shapes, dump("pq", shapes)):
        f = fields(line)
        dsub, cols, stride = d // M, int(f["cols"]), int(f["stride"])
        group, ngroups, lds = int(f["group"]), int(f["ngroups"]), int(f["lds"])
        gx, gy = (int(v) for v in f["grid"].split("x"))
        assert cols % 32 == 0 and 0 <= cols - (1 << nbits) < 32 and int(f["kq"]) == (dsub + 7) // 8 and stride % 8 == 4 and stride >= 4 * int(f["kq"])
        few, big = n < 20 and dsub % 4 == 0, pq_lds(1, cols, stride) > LDS_LIMIT
        assert (f["route"] == "loop") == (few or big), line
        seen[f["route"]] += 1
        if f["route"] == "loop":
            assert (group, ngroups, lds, gx, gy) == (1, M, 0, 1, 1) and line.endswith("why=" + (WHY_FEW if few else WHY_LDS)), line
            continue
        assert lds == pq_lds(group, cols, stride) and lds <= LDS_LIMIT, line
        assert group * ngroups >= M > group * (ngroups - 1) and 1 <= group <= min(M, (32 + dsub - 1) // dsub), line
        assert 1 <= gx <= (n + 127) // 128 and gy == ngroups, line
        assert f["vec"] == "0" or (dsub % 4 == 0 and d % 4 == 0), line
        seen["halved"] += group < min(M, (32 + dsub - 1) // dsub)
        seen["ragged"] += M % group != 0
    assert all(seen.values()), seen


def test_moments_plan_invariants(dump):
    shapes = [(n, d, d2, sym, kr, fs) for n in (1, 31, 32, 33, 127, 128, 4099, 32768, 70001) for d in (1, 127, 128, 129, 300, 960)
              for sym, d2 in ((1, 0), (0, d), (0, 129)) for kr in (0, 16, 32, 64) for fs in (0, 1, 7, 4096)]
    for (n, dx, dy, sym, fkr, fs), line in zip(shapes, dump("mom", shapes)):
        f = {k: v for k, v in fields(line).items() if k != "tiles"}
        f = {k: int(v) for k, v in f.items()}
        tx, ty = (dx + 127) // 128, ((dx if sym else dy) + 127) // 128
        assert f["kr"] == (fkr or 32) and f["pairs"] == (tx * (tx + 1) // 2 if sym else tx * ty), line
        assert f["slice_len"] % f["kr"] == 0 and (f["S"] - 1) * f["slice_len"] < n <= f["S"] * f["slice_len"], line
        assert f["scratch"] == f["S"] * f["pairs"] * 65536 and f["lds"] == 4 * f["kr"] * 128 * 4 <= LDS_LIMIT, line
        assert f["col_slices"] * f["col_slice_len"] >= n > (f["col_slices"] - 1) * f["col_slice_len"] and f["col_slices"] <= 4096, line
        assert f["col_slice_len"] % 4 == 0
        if fs:
            assert f["S"] <= fs, line
        else:               # the plan's own choice: at most two workgroups per CU, slices of at least four strips while n allows
            assert f["S"] == 1 or (f["S"] * f["pairs"] <= 512 and f["slice_len"] >= 4 * f["kr"]), line


def test_kmeans_update_plan_invariants(dump):
    shapes = [(n, k, d) for n in (1, 2, 3, 255, 256, 257, 65536, 65537, (1 << 31) - 1) for k in (1, 2, 3, 256, 257, 1 << 20)
              for d in (1, 4, 63, 64, 65, 128, 255, 256, 257, 300, 2048)]
    for (n, k, d), line in zip(shapes, dump("km", shapes)):
        f = fields(line)
        row_bits, key_bits = int(f["key_row_bits"]), int(f["key_bits"])
        gx, gy = (int(v) for v in f["grid"].split("x"))
        assert key_bits <= 64 and n - 1 < 1 << row_bits and k - 1 < 1 << (key_bits - row_bits), line
        assert (f["packed"] == "1") == (d < 64), line
        if d < 64:
            assert gx * 256 >= k * d > (gx - 1) * 256 and f["kernel"] == "kmeans_update_packed_kernel", line
        else:
            assert gx == k and gy * int(f["waves"]) * 64 >= d and 1 <= int(f["waves"]) <= 4 and f["kernel"] == "kmeans_update_kernel", line
            assert (gy - 1) * int(f["waves"]) * 64 < d, line
