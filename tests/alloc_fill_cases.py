"""Cases and runner of tests/test_alloc_fill_gpu.py — TEST INFRASTRUCTURE, no tests here.

What is checked: a result must not depend on what device memory held before the call.  The context option
debug_alloc_fill makes every block the allocators hand out (pool_alloc over its whole capacity, parked or fresh; every
device_alloc; the lazily allocated pinned staging) start as a chosen 32-bit word, and debug_alloc_filled counts the blocks.

A CASE is a function run(ctx) → dict of everything observable (arrays, numbers, nested dicts and lists of them): it
creates its own objects, performs one entry point or a short sequence, closes everything.  freeze() turns what it returns
into {name: bytes | int}, which is what is compared.  CASES maps a name to (run, verify); verify(raw, oracle), where there
is one, holds the ZERO-filled run to an independent reference of the tree with that reference's own tolerance, so that
"equal to the zero-filled run" is not merely self-agreement.

check_case runs a case under these fills, in this order, on one context, with debug_alloc_filled reset before each run:

  Z, twice   -1 (zeros)          the two runs are equal bit for bit
  A          word 0x00000001     bit for bit equal to Z
  N          word 0x7FC00001     bit for bit equal to Z
  D          word 0x7FF80001     bit for bit equal to Z

Fill A reads as the integer 1 in every width, as a set flag byte, as key 1 and as a denormal in either float width; read
as an index it stays inside any array of two elements: a dependence on leftovers shows as a wrong count, flag, key, pad or
validity byte, not as a wild address.  Fill N is a quiet NaN as a float: a leaked read into a sum, a maximum taken with
`<` or a mean poisons the output.  Two such words read as a double are NOT a NaN (the exponent field is 0x7FC, not 0x7FF)
but a finite number near 2^1021, which overflows the first product it enters; fill D is the word whose pair is a quiet NaN
as a double too, and most of what this library keeps on the device is float64.  N and D run only after A has passed,
inside the same function, so that a failing A assertion stops the case: a finding under A is fixed before that case ever
runs under N or D.  Under every fill the case must have made the allocators fill at least one block; a case that
allocates nothing on the device is listed in NO_DEVICE_ALLOCATION with the reason instead.  Keys of a case's dict that
begin with "_" are for verify alone and are not compared between the runs."""
import functools

import numpy as np

from tests import helpers

FILL_ZERO, FILL_ONE, FILL_NAN, FILL_NAN64 = -1, 0x00000001, 0x7FC00001, 0x7FF80001
assert np.isnan(np.array([FILL_NAN], dtype=np.uint32).view(np.float32)[0])
assert np.array([FILL_NAN, FILL_NAN], dtype=np.uint32).view(np.float64)[0] > 2.0 ** 1020  # finite, and huge
assert np.isnan(np.array([FILL_NAN64], dtype=np.uint32).view(np.float32)[0])
assert np.isnan(np.array([FILL_NAN64, FILL_NAN64], dtype=np.uint32).view(np.float64)[0])
FILLS = (("A", FILL_ONE), ("N", FILL_NAN), ("D", FILL_NAN64))  # what follows the two zero-filled runs, in this order

CASES = {}                 # name → (run, verify or None)
NO_DEVICE_ALLOCATION = {}  # name → why the case fills nothing (every case here allocates: none so far)

EXP = ("exponential", 1.0, 1.0)
NDT_LOSSES = (None, EXP, ("huber", 1.2))       # those of tests/test_gpu_parity.py
RTOL_F64, RTOL_F32, RTOL_F32_REPROJ = 1e-10, 3e-6, 2e-6  # tests/test_gpu_parity.py: kernels against the CPU oracle
# The two fp32 bounds were measured at that file's shapes (tens of thousands of items, one voxel per 20) and hold the
# 40 000-item cases here as they stand.  Fewer items average less, and what a float rounding does to a sum is then a
# property of the data: of the cancellation in p - mu and u - projection, of an exponential weight near float's range.
# The smaller fp32 cases are held to  base + 4 E (+ E_proj)  with both terms from the fp64 ORACLE alone (_f32_bound):
#   E       the oracle's sums over the inputs rounded to float against its sums over the inputs, in the measure of
#           helpers.assert_normal_equations_close: what ONE rounding of every stored value does on this data.  The device
#           rounds p and mu likewise (and A where this sample rounds S) and then forms R p + t - mu in float, three more
#           roundings of operands of the same magnitude: 4 E covers the five with the sample's two.
#   E_proj  reprojection only: the residual a - b, a = x / z of the camera-frame point, b = (u - cx) / fx, cancels, and the
#           float error of a follows the magnitude of X, not of the residual.  With u = 2^-24: x and z are three products
#           and three additions each, every partial sum at most Sx = sum_j |R_0j X_j| + |t_0| (Sz likewise), so
#           dx <= 6 u Sx, dz <= 6 u Sz; da <= dx / z + |x| dz / z^2 + u |a|; db <= 2 u |b|.  The oracle's sums with every
#           u moved by (da + db) fx and every v likewise, both relative signs, against its sums: the worse of the two.
# A term whose loss weight lies below float's smallest normal may come out as zero: n FLT_MIN times the unweighted scale
# is allowed on top (_assert_f32_close).  The loss's VALUE is a difference of float numbers as large as the loss's own
# constants whatever the residual — c1 - c1 exp(-c2 s), 2 d sqrt(s) - d^2 — so every item's cost may be off by the
# roundings of those: 2 u c1 (the exponential and the difference), 4 u d^2 (at the threshold the two terms are 2 d^2 and
# d^2; the root, the product, the difference), u = 2^-24; n of them on the cost (_loss_rounding).  Nothing in a bound comes
# from the code under test.
FLT_MIN = float(np.finfo(np.float32).tiny)
R_TEST = helpers.rot_xyz(0.01, -0.02, 0.05)
T_TEST = np.array([-0.1, 0.05, 0.2])
R2_TEST = np.array([[np.cos(0.07), -np.sin(0.07)], [np.sin(0.07), np.cos(0.07)]])
T2_TEST = np.array([-0.15, 0.1])
R_REPROJ = helpers.rot_xyz(0.0, 0.01, -0.08)
T_REPROJ = np.array([0.08, -0.1, 0.4])
POSE = (helpers.rot_xyz(0.01, -0.02, 0.05), np.array([0.1, -0.2, 0.05]))  # tests/test_voxel_store_life.py


# ---------------------------------------------------------------------------------------------------- the runner

def freeze(value, prefix="", out=None):
    """what a case returns → {name: bytes | int}; arrays keep their type and shape, NaNs compare by their bits"""
    out = {} if out is None else out
    if isinstance(value, dict):
        for k in value:
            if not str(k).startswith("_"):
                freeze(value[k], "%s.%s" % (prefix, k) if prefix else str(k), out)
    elif isinstance(value, (list, tuple)):
        for k, v in enumerate(value):
            freeze(v, "%s[%d]" % (prefix, k), out)
    elif isinstance(value, np.ndarray):
        a = np.ascontiguousarray(value)
        out[prefix] = ("%s%r" % (a.dtype.str, a.shape)).encode() + a.tobytes()
    elif isinstance(value, (bool, int, np.integer, np.bool_)):
        out[prefix] = int(value)
    elif isinstance(value, (float, np.floating)):
        out[prefix] = np.float64(value).tobytes()
    elif isinstance(value, (bytes, str)) or value is None:
        out[prefix] = value if isinstance(value, bytes) else repr(value).encode()
    else:
        raise TypeError("%s: a case returned a %s" % (prefix, type(value).__name__))
    return out


def run_under(ctx, run, fill):
    """one run of a case with every handed-out block filled with `fill` → (what it returned, blocks filled)"""
    ctx.set_option("debug_alloc_filled", 0)
    ctx.set_option("debug_alloc_fill", fill)
    try:
        raw = run(ctx)
    finally:
        ctx.set_option("debug_alloc_fill", 0)
    return raw, ctx.get_option("debug_alloc_filled")


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def _unpacked_scales(want, dim):
    """the scales of helpers.assert_normal_equations_close → (H, g, cost as unpacked, scale of H, scale of g)"""
    H, g, c = helpers.unpack(want, dim)
    d = np.sqrt(np.maximum(np.diag(H), 0.0))
    return H, g, c, np.outer(d, d) + 1e-300, d * max(np.max(np.abs(g) / (d + 1e-300)), 1e-300) + 1e-300


def _scaled_error(got, want, dim):
    """the largest of the three errors helpers.assert_normal_equations_close compares with its rtol"""
    Hw, gw, cw, sH, sg = _unpacked_scales(want, dim)
    Hg, gg, cg = helpers.unpack(got, dim)
    return max(np.max(np.abs(Hg - Hw) / sH), np.max(np.abs(gg - gw) / sg), abs(cg - cw) / max(abs(cw), 1e-300))


def _f32_bound(base, n, want, samples, dim):
    """the bound of an fp32 dataset against the fp64 oracle's `want` (see RTOL_F32): samples = the oracle's sums over
    perturbed inputs, [(factor, sums), ...]"""
    if n >= 40_000:
        return base
    return base + sum(factor * _scaled_error(sums, want, dim) for factor, sums in samples)


def _loss_rounding(loss):
    """what the float evaluation of one item's loss value may be off by, whatever the residual (see RTOL_F32)"""
    if loss is None:
        return 0.0
    return 2.0 ** -24 * (2.0 * loss[1] if loss[0] == "exponential" else 4.0 * loss[1] * loss[1])


def _assert_f32_close(got, want, unweighted, dim, rtol, n, where, loss=None):
    """helpers.assert_normal_equations_close with n FLT_MIN of the loss-free sums' scales allowed on top, and n roundings
    of the loss's value on the cost"""
    Hw, gw, cw, sH, sg = _unpacked_scales(want, dim)
    _, _, c0, sH0, sg0 = _unpacked_scales(unweighted, dim)
    Hg, gg, cg = helpers.unpack(got, dim)
    tiny = n * FLT_MIN
    print("%s: scaled error %.3g, bound %.3g" % (where, _scaled_error(got, want, dim), rtol))
    assert np.all(np.abs(Hg - Hw) <= rtol * sH + tiny * sH0), (where, "H", rtol)
    assert np.all(np.abs(gg - gw) <= rtol * sg + tiny * sg0), (where, "g", rtol)
    assert abs(cg - cw) <= rtol * abs(cw) + tiny * abs(c0) + n * _loss_rounding(loss), (where, "cost", rtol, cg, cw)


def check_case(ctx, name, oracle=None, fills=FILLS):
    """The steps of the module docstring for one case.  fills: what follows the two zero-filled runs, in order."""
    run, verify = CASES[name]

    def step(label, fill):
        raw, filled = run_under(ctx, run, fill)
        if name in NO_DEVICE_ALLOCATION:
            assert filled == 0, (name, label, "fills blocks after all: take it out of NO_DEVICE_ALLOCATION", filled)
        else:
            assert filled > 0, (name, label, "the case made no allocator fill a block")
        return raw, filled

    z_raw, filled = step("Z", FILL_ZERO)
    if verify is not None:
        verify(z_raw, oracle)
    z = freeze(z_raw)
    assert z, (name, "the case returned nothing")
    again = differing(z, freeze(step("Z again", FILL_ZERO)[0]))
    assert not again, (name, "two zero-filled runs differ", again)
    for label, fill in fills:  # in order: a failing A stops the case before N and D
        wrong = differing(z, freeze(step(label, fill)[0]))
        assert not wrong, (name, "fill %s (word 0x%08X) changes the result" % (label, fill & 0xFFFFFFFF), wrong)
    return len(z), filled


def _case(name, verify=None):
    def register(run):
        assert name not in CASES, name
        CASES[name] = (run, verify)
        return run
    return register


def _report(rep):
    """a solve's report without `launches` and `fallback`: on a GPU that other processes use the one-launch loop may give
    way to the launch-per-iteration loop, which is no property of the memory the call was handed"""
    return {k: rep[k] for k in ("iterations", "ok", "printed_cost", "last_cost", "final_lambda", "cost_history")}


def _solve(out):
    R, t, rep = out
    return {"R": R, "t": t, "report": _report(rep)}


# ------------------------------------------------------------------------------------------------ flat datasets

@functools.lru_cache(maxsize=None)
def _ndt_planes(n):
    from nonlinear_optimizer_for_slam_amd import synth
    return synth.ndt_planes(n, max(1, n // 20))


@functools.lru_cache(maxsize=None)
def _reproj_planes(n):
    from nonlinear_optimizer_for_slam_amd import synth
    planes = synth.reproj_planes(n)
    if n > 200:
        planes[2, 50:150] = -2.0  # behind the camera: dropped by the depth test
    return planes


def _records(planes):
    """the planes as AoS records with 8 bytes of padding behind every record → (bytes, stride, offsets)"""
    k, n = planes.shape
    rec = np.full((n, k + 1), -7.0)
    rec[:, :k] = planes.T
    return rec.tobytes(), 8 * (k + 1), [8 * f for f in range(k)]


def _flat_ndt(dtype, n, tile):
    from nonlinear_optimizer_for_slam_amd import NdtDataset, api
    solves = n >= 1000

    def run(ctx):
        planes = _ndt_planes(n)
        out = {}
        with ctx.options(**({} if tile is None else {"tile_log2": tile})):
            routes = {"planes": NdtDataset.from_planes(ctx, planes, dtype),
                      "records": NdtDataset.from_records(ctx, *_records(planes), dtype)}
        for route, ds in routes.items():
            o = out[route] = {"len": len(ds), "stream_bytes": ds.stream_bytes, "download": api.download(ds)}
            for k, loss in enumerate(NDT_LOSSES):
                o["accumulate6_%d" % k] = ds.accumulate6(R_TEST, T_TEST, loss)
                o["accumulate3_%d" % k] = ds.accumulate3(R2_TEST, T2_TEST, loss)
            if solves:
                o["solve6"] = _solve(ds.solve6(np.eye(3), np.zeros(3), EXP, max_iterations=40))
                o["solve3"] = _solve(ds.solve3(np.eye(2), np.zeros(2), EXP, max_iterations=40))
            ds.close()
        return out

    def verify(raw, oracle):
        planes = _ndt_planes(n)
        assert freeze(raw["planes"]) == freeze(raw["records"])  # two ingestion routes, one dataset
        o = raw["planes"]
        stored = planes[:3] if dtype == "f64" else planes[:3].astype(np.float32).astype(np.float64)
        assert o["download"][:3].tobytes() == stored.tobytes()
        rounded = planes.astype(np.float32).astype(np.float64)
        for dim, key, fn, pose in ((6, "accumulate6_%d", oracle.ndt6_accumulate, (R_TEST, T_TEST)),
                                   (3, "accumulate3_%d", oracle.ndt3_accumulate, (R2_TEST, T2_TEST))):
            for k, loss in enumerate(NDT_LOSSES):
                want = fn(planes, *pose, loss)
                if dtype == "f64":
                    helpers.assert_normal_equations_close(o[key % k], want, dim, RTOL_F64)
                    continue
                rtol = _f32_bound(RTOL_F32, n, want, [(4.0, fn(rounded, *pose, loss))], dim)
                _assert_f32_close(o[key % k], want, fn(planes, *pose, None), dim, rtol, n, (n, key % k), loss)
        if solves and dtype == "f64":  # the final pose of the fp64 loop: 1e-6, tests/test_gpu_parity.py
            want = oracle.ndt6_solve(planes, np.zeros(3), np.eye(3), loss=EXP, linear_solver=1)
            dt, dq = helpers.pose_delta(o["solve6"]["R"].reshape(3, 3), o["solve6"]["t"], want["R"], want["t"])
            assert dt < 1e-6 and dq < 1e-6 and o["solve6"]["report"]["iterations"] == want["iterations"], (dt, dq)

    return run, verify


def _flat_reproj(dtype, n, tile):
    from nonlinear_optimizer_for_slam_amd import ReprojDataset, api, synth
    losses = (None, EXP, ("huber", synth.REPROJ_HUBER_THRESHOLD))
    solves = n >= 1000

    def run(ctx):
        planes = _reproj_planes(n)
        out = {}
        with ctx.options(**({} if tile is None else {"tile_log2": tile})):
            routes = {"planes": ReprojDataset.from_planes(ctx, planes, dtype),
                      "records": ReprojDataset.from_records(ctx, *_records(planes), dtype)}
        for route, ds in routes.items():
            o = out[route] = {"len": len(ds), "stream_bytes": ds.stream_bytes, "download": api.download(ds)}
            for k, loss in enumerate(losses):
                o["accumulate_%d" % k] = ds.accumulate(R_REPROJ, T_REPROJ, synth.REPROJ_INTR4, loss)
            if solves:
                o["solve"] = _solve(ds.solve(np.eye(3), np.zeros(3), synth.REPROJ_INTR4, losses[2], max_iterations=40))
            ds.close()
        return out

    def verify(raw, oracle):
        planes = _reproj_planes(n)
        assert freeze(raw["planes"]) == freeze(raw["records"])
        o = raw["planes"]
        stored = planes if dtype == "f64" else planes.astype(np.float32).astype(np.float64)
        assert o["download"].tobytes() == stored.tobytes()
        def sums(p, loss):
            return oracle.reproj_accumulate(p, R_REPROJ, T_REPROJ, synth.REPROJ_INTR4, loss)

        rounded = planes.astype(np.float32).astype(np.float64)
        u32, intr = 2.0 ** -24, synth.REPROJ_INTR4
        cam = R_REPROJ @ planes[:3] + T_REPROJ[:, None]
        reach = np.abs(R_REPROJ) @ np.abs(planes[:3]) + np.abs(T_REPROJ)[:, None]  # Sx, Sy, Sz
        z = np.where(cam[2] > 0.03, cam[2], np.inf)  # the depth test drops the rest: they take no step
        step = np.zeros((2, planes.shape[1]))
        for axis in (0, 1):
            a_, b_ = cam[axis] / z, (planes[3 + axis] - intr[2 + axis]) * intr[axis]
            da = 6.0 * u32 * reach[axis] / z + np.abs(cam[axis]) * 6.0 * u32 * reach[2] / (z * z) + u32 * np.abs(a_)
            step[axis] = (da + 2.0 * u32 * np.abs(b_)) / intr[axis]
        moved = []
        for sign in (1.0, -1.0):
            m = planes.copy()
            m[3], m[4] = planes[3] + step[0], planes[4] + sign * step[1]
            moved.append(m)
        for k, loss in enumerate(losses):
            want = sums(planes, loss)
            if dtype == "f64":
                helpers.assert_normal_equations_close(o["accumulate_%d" % k], want, 6, RTOL_F64)
                continue
            e_proj = max(_scaled_error(sums(m, loss), want, 6) for m in moved)
            rtol = _f32_bound(RTOL_F32_REPROJ, n, want, [(4.0, sums(rounded, loss))], 6) + (e_proj if n < 40_000 else 0.0)
            _assert_f32_close(o["accumulate_%d" % k], want, sums(planes, None), 6, rtol, n, (n, "accumulate_%d" % k), loss)

    return run, verify


for _maker, _kind in ((_flat_ndt, "ndt"), (_flat_reproj, "reproj")):
    for _n in (1, 513, 1000, 40_000):  # 40 000: the streamed one-launch loop and its partial rows
        for _dtype, _tile in (("f64", None), ("f32", None), ("f32", 0), ("f32", 10)):  # f32: default, planar, tiles of 1024
            _name = "flat_%s_%s%s_%d" % (_kind, _dtype, "" if _tile is None else "_tile%d" % _tile, _n)
            CASES[_name] = _maker(_dtype, _n, _tile)


# --------------------------------------------------------------------------------------------- indexed datasets

@functools.lru_cache(maxsize=None)
def _indexed_inputs(n=1000, v=7, k=2, seed=1007, frac_missing=0.1):
    """tests/test_indexed.py's generator → (points [3, n], ids [k, n], means, S, the equivalent flat planes)"""
    rng = np.random.default_rng(seed)
    means = rng.uniform(-20, 20, size=(v, 3))
    S = rng.normal(size=(v, 3, 3)) * 3.0
    idx = rng.integers(0, v, size=(k, n)).astype(np.int32)
    idx[rng.uniform(size=(k, n)) < frac_missing] = -1
    pts = (means[np.maximum(idx[0], 0)] + rng.normal(scale=0.3, size=(n, 3))).T.copy()
    cols = []
    for kk in range(k):
        ok = idx[kk] >= 0
        cols.append(np.concatenate([pts[:, ok], means[idx[kk, ok]].T, S[idx[kk, ok]].reshape(-1, 9).T], axis=0))
    return pts, idx, means, S, np.concatenate(cols, axis=1)


def _indexed(dtype, sort):
    from nonlinear_optimizer_for_slam_amd import NdtIndexedDataset, api

    def run(ctx):
        pts, idx, means, S, _ = _indexed_inputs()
        ds = NdtIndexedDataset.from_arrays(ctx, pts, idx, means, S, dtype, sort)
        out = {"len": len(ds), "n_slots": ds.n_slots, "n_voxels": ds.n_voxels, "ids": ds.ids(), "table": ds.table(),
               "points": api.download(ds)}
        for k, loss in enumerate(NDT_LOSSES):
            out["accumulate6_%d" % k] = ds.accumulate6(R_TEST, T_TEST, loss)
            out["accumulate3_%d" % k] = ds.accumulate3(R2_TEST, T2_TEST, loss)
        ds.close()
        return out

    def verify(raw, oracle):
        pts, idx, means, S, flat = _indexed_inputs()
        rtol = 1e-10 if dtype == "f64" else 1e-4  # tests/test_indexed.py
        for k, loss in enumerate(NDT_LOSSES):
            helpers.assert_normal_equations_close(raw["accumulate6_%d" % k], oracle.ndt6_accumulate(flat, R_TEST, T_TEST, loss), 6, rtol)
            helpers.assert_normal_equations_close(raw["accumulate3_%d" % k], oracle.ndt3_accumulate(flat, R2_TEST, T2_TEST, loss), 3, rtol)
        assert raw["ids"].shape == idx.shape and raw["table"].shape == (means.shape[0], 16)
        assert int((raw["ids"] < 0).sum()) == int((idx < 0).sum())  # the absent ids stay absent, pads are not counted
        if not sort:
            stored = pts if dtype == "f64" else pts.astype(np.float32).astype(np.float64)
            assert np.array_equal(raw["ids"], idx) and raw["points"].tobytes() == stored.tobytes()
        if dtype == "f64":
            assert raw["table"][:, :3].tobytes() == means.tobytes()

    return run, verify


for _dtype in ("f64", "f32"):
    for _sort in (True, False):
        CASES["indexed_%s_%s" % (_dtype, "sorted" if _sort else "unsorted")] = _indexed(_dtype, _sort)


# ------------------------------------------------------------------------------------------------------- NdtMap

@functools.lru_cache(maxsize=None)
def _map_inputs(v=300, seed=31):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-10, 10, size=(v, 3))
    S = rng.normal(size=(v, 3, 3)) * 3.0
    valid = (np.arange(v) % 11 != 5).astype(np.uint8)
    scans = tuple(means[rng.integers(0, v, size=n)] + rng.normal(scale=0.6, size=(n, 3)) for n in (1, 257, 1025))
    return means, S, valid, scans


def _nearest_two(means, valid, moved, radius_sq):
    """→ (matches, matched points): up to two nearest valid voxel means within the radius, by brute force"""
    d = ((moved[:, None, :] - means[None, valid != 0, :]) ** 2).sum(axis=2)
    within = np.sort(d, axis=1)[:, :2] < radius_sq
    return int(within.sum()), int(within.any(axis=1).sum())


def _dataset_out(ds, n_matches, indexed=False):
    from nonlinear_optimizer_for_slam_amd import api
    out = {"n": n_matches, "len": len(ds), "planes": api.download(ds), "accumulate6": ds.accumulate6(POSE[0], POSE[1], EXP),
           "accumulate3": ds.accumulate3(R2_TEST, T2_TEST, EXP)}
    if indexed:
        out.update(ids=ds.ids(), table=ds.table(), n_voxels=ds.n_voxels)
    ds.close()
    return out


@_case("ndt_map_given", verify=lambda raw, oracle: _verify_map_given(raw))
def _run_map_given(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    means, S, valid, scans = _map_inputs()
    gm = api.NdtMap(ctx, means, S, valid, 1.0)
    out = {"len": len(gm)}
    for pts in scans:
        sc = api.Scan(ctx, pts)
        o = out["scan_%d" % len(pts)] = {}
        for dtype in ("f64", "f32"):
            o["match_" + dtype] = _dataset_out(*gm.match(sc, POSE[0], POSE[1], 2, dtype))
            for sort in (False, True):
                o["match_indexed_%s_%d" % (dtype, sort)] = _dataset_out(*gm.match_indexed(sc, POSE[0], POSE[1], 2, dtype, sort), indexed=True)
        for k, loss in enumerate(NDT_LOSSES):
            o["score_%d" % k] = list(gm.score(sc, POSE[0], POSE[1], loss))
        sc.close()
    gm.close()
    return out


def _verify_map_given(raw):
    means, S, valid, scans = _map_inputs()
    assert raw["len"] == int(valid.sum())
    total = 0
    for pts in scans:
        o = raw["scan_%d" % len(pts)]
        matches, points = _nearest_two(means, valid, pts @ POSE[0].T + POSE[1], 1.0)
        total += matches
        for key in o:
            if key.startswith("match"):
                assert o[key]["n"] == matches, (key, o[key]["n"], matches)
            else:
                assert o[key][:2] == [matches, points], (key, o[key], matches, points)
        cost = o["match_f64"]["accumulate6"][27]  # the score sums the same terms in another order (tests/test_score_batch.py)
        assert abs(o["score_1"][2] - cost) <= 2 * len(pts) * 2.0 ** -52 * cost, (o["score_1"], cost)
    assert total > 500


@functools.lru_cache(maxsize=None)
def _build_points(n=6000, seed=32):
    rng = np.random.default_rng(seed)
    centres = rng.integers(-6, 6, size=(150, 3)) + 0.5
    return centres[rng.integers(0, 150, size=n)] + rng.uniform(-0.45, 0.45, size=(n, 3))


def _map_build(compact):
    def run(ctx):
        from nonlinear_optimizer_for_slam_amd import api
        with ctx.options(map_compact_keys=compact):
            gm, stats = api.NdtMap.build(ctx, _build_points(), 1.0, 1.0)
            quiet, none = api.NdtMap.build(ctx, _build_points(), 1.0, 1.0, return_stats=False)
        out = {"len": len(gm), "len_quiet": len(quiet), "stats": stats}
        assert none is None
        gm.close(), quiet.close()
        return out

    def verify(raw, oracle):
        pts = _build_points()
        cells, inverse, counts = np.unique(np.floor(pts).astype(np.int64), axis=0, return_inverse=True, return_counts=True)
        st = raw["stats"]
        at = np.lexsort(st["cells"].T[::-1])  # whatever the build's order is, cell by cell
        assert np.array_equal(st["cells"][at], cells) and np.array_equal(st["counts"][at], counts)
        sums = np.zeros((cells.shape[0], 3))
        np.add.at(sums, inverse.reshape(-1), pts)
        ok = st["valid"][at]
        assert np.array_equal(ok, counts >= 5)  # five points make a voxel; these clouds fill their cells: none is degenerate
        np.testing.assert_allclose(st["means"][at][ok], (sums / counts[:, None])[ok], rtol=0, atol=1e-12)  # tests/voxel_store_model.py
        assert raw["len"] == raw["len_quiet"] == int(ok.sum())

    return run, verify


for _compact in (0, 1):
    CASES["ndt_map_build_compact%d" % _compact] = _map_build(_compact)


# --------------------------------------------------------------------------------------------------------- Scan

@functools.lru_cache(maxsize=None)
def _scan_points(n, specials=False):
    from tests import place_inputs
    return place_inputs.scan_points(n, 64, 128, seed=n, specials=specials)[0] if n else np.zeros((0, 3))


def _scan(n):
    def run(ctx):
        from nonlinear_optimizer_for_slam_amd import api
        pts = _scan_points(n)
        rng = np.random.default_rng(n)
        times, twist = rng.uniform(0.0, 1.0, size=n), np.array([0.8, -0.1, 0.02, 0.01, -0.02, 0.15])
        out = {}
        for name, kw in (("plain", {}), ("sorted", {"sort_cell": 1.0}), ("filtered", {"filter_voxel": 2.0}),
                         ("both", {"sort_cell": 1.0, "filter_voxel": 2.0})):
            sc = api.Scan(ctx, pts, **kw)
            o = out[name] = {"len": len(sc), "points": sc.points(), "order": sc.order}
            for what, made in (("filtered", sc.filtered(4.0)), ("deskewed", sc.deskewed(times, twist))):
                o[what] = {"len": len(made), "points": made.points(), "order": made.order}
                made.close()
            for rings, sectors in ((20, 60), (64, 128)):
                desc, used = sc.descriptor(rings, sectors)
                o["descriptor_%d_%d" % (rings, sectors)] = {"desc": desc, "used": used}
            sc.close()
        special = api.Scan(ctx, _scan_points(n, specials=True))  # NaN and infinite coordinates among the points
        for rings, sectors in ((20, 60), (64, 128)):
            desc, used = special.descriptor(rings, sectors)
            out["special_descriptor_%d_%d" % (rings, sectors)] = {"desc": desc, "used": used}
        special.close()
        return out

    def verify(raw, oracle):
        from tests import place_inputs
        from tests.voxel_store_sequences import first_per_voxel
        pts = _scan_points(n)
        assert raw["plain"]["points"].tobytes() == pts.tobytes()
        assert np.array_equal(raw["plain"]["order"], np.arange(n))
        assert raw["filtered"]["points"].tobytes() == first_per_voxel(pts, 2.0).tobytes() if n else raw["filtered"]["len"] == 0
        assert raw["plain"]["filtered"]["points"].tobytes() == first_per_voxel(pts, 4.0).tobytes() if n else True
        for name in ("plain", "sorted", "filtered", "both"):
            o = raw[name]
            assert o["points"].tobytes() == pts[o["order"]].tobytes(), name  # `order` names the stored points
            assert np.array_equal(o["deskewed"]["order"], o["order"]) and o["deskewed"]["len"] == o["len"], name
            for rings, sectors in ((20, 60), (64, 128)):  # bit for bit: tests/test_place_descriptor.py
                desc, used = place_inputs.descriptor(o["points"], rings, sectors)
                got = o["descriptor_%d_%d" % (rings, sectors)]
                assert got["used"] == used and got["desc"].tobytes() == desc.tobytes(), (name, rings, sectors)
        for rings, sectors in ((20, 60), (64, 128)):
            desc, used = place_inputs.descriptor(_scan_points(n, specials=True), rings, sectors)
            got = raw["special_descriptor_%d_%d" % (rings, sectors)]
            assert got["used"] == used and got["desc"].tobytes() == desc.tobytes(), (rings, sectors)

    return run, verify


for _n in (0, 1, 257, 5000):
    CASES["scan_%d" % _n] = _scan(_n)


@_case("descriptor", verify=lambda raw, oracle: _verify_descriptor(raw))
def _run_descriptor(ctx):
    """Scan.descriptor alone, at both parameter sets: the case of the scratch mutation (the zeroing of the key array in
    front of place_descriptor_kernel taken out must fail this under fill A)"""
    from nonlinear_optimizer_for_slam_amd import api
    out = {}
    for n in (1, 257, 5000):
        sc = api.Scan(ctx, _scan_points(n, specials=True))
        for rings, sectors in ((20, 60), (64, 128)):
            desc, used = sc.descriptor(rings, sectors)
            out["%d_%d_%d" % (n, rings, sectors)] = {"desc": desc, "used": used}
        sc.close()
    return out


def _verify_descriptor(raw):
    from tests import place_inputs
    for n in (1, 257, 5000):
        for rings, sectors in ((20, 60), (64, 128)):
            desc, used = place_inputs.descriptor(_scan_points(n, specials=True), rings, sectors)
            got = raw["%d_%d_%d" % (n, rings, sectors)]
            assert got["used"] == used and got["desc"].tobytes() == desc.tobytes(), (n, rings, sectors)


# ----------------------------------------------------------------------------------------------------- VoxelMap

def _voxel_scans(ctx, api, sizes=(1, 63, 513), seed=1001):
    from tests import voxel_store_sequences as vs
    rng = np.random.default_rng(seed)
    return [api.Scan(ctx, rng.uniform(vs.LO, vs.HI, size=(n, 3))) for n in sizes]


def _register_out(result):
    R, t, reports = result
    return {"R": R, "t": t, "reports": reports}


def _run_program(ctx, api, ops, A, B):
    """one program of tests/voxel_store_sequences.py on the stores A and B → what every call returned"""
    returned, to_close = [], []
    for op in ops:
        kind, vm = op["op"], (B if op.get("store") == "B" else A)
        if kind == "insert":
            got = vm.insert(op["points"])
        elif kind == "insert_scan":
            sc = api.Scan(ctx, op["points"], sort_cell=op["sort_cell"], filter_voxel=op["filter_voxel"])
            to_close.append(sc)
            got = A.insert_scan(sc, op["R"], op["t"])
        elif kind == "prune":
            got = vm.prune(center=op["center"], half_extent=op["half_extent"], max_age=op["max_age"])
        elif kind == "carve":
            sc = api.Scan(ctx, op["points"])
            to_close.append(sc)
            removed, info = vm.carve(sc, op["R"], op["t"], counts=True, **op["how"])
            got = {"removed": removed, "skipped": info["skipped"], "crossings": info["crossings"], "hits": info["hits"]}
        elif kind == "merge":
            got = A.merge(B, op["R"], op["t"])
        else:
            empty = api.VoxelMap(ctx, op["res"], 1.0)
            to_close.append(empty)
            got = A.merge(empty, op["R"], op["t"])
        returned.append(got)
    for h in to_close:
        h.close()
    return returned


def _store_out(vm):
    return {"stats": vm.stats(), "memory": vm.memory(), "len": len(vm), "n_valid": vm.n_valid, "n_points": vm.n_points}


PROGRAM = (1, 1.0, 0.5)  # seed and resolutions: the merges go into the coarser grid


@_case("voxel_map", verify=lambda raw, oracle: _verify_voxel_map(raw))
def _run_voxel_map(ctx):
    """growth from 16 slots, insert, insert_scan, prune, carve and merge by one seeded program; then the state calls, the
    readers and the batched registrations on the live store"""
    from nonlinear_optimizer_for_slam_amd import api
    from tests import voxel_store_sequences as vs
    ops = vs.program(*PROGRAM)
    A, B = api.VoxelMap(ctx, PROGRAM[1], 1.0, capacity=0), api.VoxelMap(ctx, PROGRAM[2], 1.0)
    out = {"returned": _run_program(ctx, api, ops, A, B), "A": _store_out(A), "B": _store_out(B)}
    # state: export (whole, and what a box would remove), restore, from_state, add, coarsened, snapshot
    whole = A.export()
    gone = A.export(center=(0.0, 0.0, 0.0), half_extent=(4.0, 4.0, 2.0), removed=True)
    out["export"], out["export_removed"] = whole, gone
    restored = api.VoxelMap(ctx, PROGRAM[1], 1.0)
    out["restore"] = {"touched": restored.restore(whole), "store": _store_out(restored)}
    twin = api.VoxelMap.from_state(ctx, whole, capacity=1 << 13)
    out["from_state"] = _store_out(twin)
    out["pruned"] = restored.prune(center=(0.0, 0.0, 0.0), half_extent=(4.0, 4.0, 2.0))
    out["add"] = {"touched": restored.add(gone), "store": _store_out(restored)}
    coarse = A.coarsened(2)
    out["coarsened"] = _store_out(coarse)
    snap = A.snapshot()
    out["snapshot_len"] = len(snap)
    # readers on the live store and, for the registrations, on the snapshot as well
    scans = _voxel_scans(ctx, api)
    big = scans[-1]
    for name, m in (("live", A), ("snapshot", snap)):
        o = out[name] = {}
        for dtype in ("f64", "f32"):
            o["match_" + dtype] = _dataset_out(*m.match(big, POSE[0], POSE[1], 2, dtype))
            o["match_indexed_" + dtype] = _dataset_out(*m.match_indexed(big, POSE[0], POSE[1], 2, dtype, sort_by_voxel=False), indexed=True)
        o["score"] = [list(m.score(big, POSE[0], POSE[1], loss)) for loss in NDT_LOSSES]
        R0, t0 = np.tile(POSE[0].reshape(9), (len(scans), 1)), np.tile(POSE[1], (len(scans), 1))
        o["register6"] = _register_out(api.register6_batch(m, scans, R0, t0, EXP, keep_multiple=4))
        o["register3"] = _register_out(api.register3_batch(m, scans, R0, t0, EXP, keep_multiple=4))
    out["match_map"] = _dataset_out(*A.match_map(B, POSE[0], POSE[1], 2, "f64"))
    rays = api.Scan(ctx, api.ray_pattern(90, np.linspace(-0.3, 0.3, 4)))
    voxels, ranges, info = A.raycast(rays, np.eye(3), np.array([0.5, 0.5, 0.25]), 30.0, points=True)
    hit = info.pop("scan")
    out["raycast"] = {"voxels": voxels, "ranges": ranges, "info": info, "points": hit.points(), "order": hit.order}
    out["A_after"] = _store_out(A)
    for h in scans + [hit, rays, snap, coarse, twin, restored, A, B]:
        h.close()
    return out


def _rows(o):
    """what the ids of a voxel-indexed dataset name: table[ids], zeros where the id is -1 → (present, rows)"""
    rows = np.zeros(o["ids"].shape + (16,))
    rows[o["ids"] >= 0] = o["table"][o["ids"][o["ids"] >= 0]]
    return o["ids"] >= 0, rows


def _verify_voxel_map(raw):
    """the calls' return values and the stores' cells, counts and means against the model of tests/voxel_store_model.py;
    the live readers against the snapshot's (bit for bit: tests/test_voxel_store_life.py)"""
    from tests import voxel_store_sequences as vs
    from tests.voxel_store_model import Model
    A, B = Model(PROGRAM[1], capacity=0), Model(PROGRAM[2])
    for op, got in zip(vs.program(*PROGRAM), raw["returned"]):
        want = vs.apply(dict(op), A, B)
        if op["op"] == "carve":
            assert (got["removed"], got["skipped"]) == tuple(want[:2]), (op["op"], got, want[:2])
            assert np.array_equal(got["crossings"], want[2]) and np.array_equal(got["hits"], want[3])
        else:
            assert got == want, (op["op"], got, want)
    for name, model in (("A", A), ("B", B)):
        st = raw[name]["stats"]
        assert np.array_equal(st["cells"], model.cells) and np.array_equal(st["counts"], model.counts), name
        ok = st["valid"]
        np.testing.assert_allclose(st["means"][ok], (model.sums[:, :3] / model.counts[:, None])[ok], rtol=0, atol=1e-12)
        assert raw[name]["memory"]["capacity"] == model.capacity and raw[name]["memory"]["epoch"] == model.epoch, name
        assert (raw[name]["len"], raw[name]["n_points"]) == (model.cells.shape[0], int(model.counts.sum())), name
    assert freeze(raw["A_after"]) == freeze(raw["A"])  # the readers leave the store alone
    assert np.array_equal(raw["export"]["cells"], A.cells) and np.array_equal(raw["export"]["counts"], A.counts)
    corner = A.cells * PROGRAM[1]  # the export's sums are about the cell corner, the model's about the origin
    np.testing.assert_allclose(corner + raw["export"]["sums"][:, :3] / A.counts[:, None], A.sums[:, :3] / A.counts[:, None], rtol=0, atol=1e-12)
    for name in ("restore", "add"):  # restored, and pruned and added back: the store again, capacity and generation aside
        assert freeze(raw[name]["store"]["stats"]) == freeze(raw["A"]["stats"]) if name == "restore" else True
        assert raw[name]["store"]["n_points"] == raw["A"]["n_points"] and raw[name]["store"]["len"] == raw["A"]["len"], name
    assert freeze(raw["from_state"]["stats"]) == freeze(raw["A"]["stats"])
    assert raw["pruned"] == raw["export_removed"]["cells"].shape[0] == raw["add"]["touched"] > 0
    assert raw["coarsened"]["n_points"] == raw["A"]["n_points"] and 0 < raw["coarsened"]["len"] < raw["A"]["len"]
    assert raw["snapshot_len"] == raw["A"]["n_valid"]
    for key, live in raw["live"].items():  # as tests/test_voxel_store_life.py compares them
        snap = raw["snapshot"][key]
        if key.startswith("match_indexed"):  # the live table is compact: the same rows under other ids
            assert (live["n"], live["len"]) == (snap["n"], snap["len"]), key
            assert live["accumulate6"].tobytes() == snap["accumulate6"].tobytes(), key
            (pl, rl), (ps, rs) = _rows(live), _rows(snap)
            assert np.array_equal(pl, ps) and rl.tobytes() == rs.tobytes(), key
        else:
            assert freeze(live) == freeze(snap), (key, differing(freeze(live), freeze(snap)))
    assert raw["live"]["match_f64"]["n"] > 100 and raw["match_map"]["n"] > 0 and raw["raycast"]["info"]["hits"] > 0


# ------------------------------------------------------------------------------------------------------ batches

@_case("solve_batches", verify=lambda raw, oracle: _verify_solve_batches(raw))
def _run_solve_batches(ctx):
    """solve6_batch and reproj_solve_batch with B = 5, one problem empty and one of a single item, and the lone solves of
    the same problems"""
    from nonlinear_optimizer_for_slam_amd import NdtDataset, ReprojDataset, api, synth
    sizes = (300, 0, 1, 513, 64)
    R0, t0 = synth.random_poses(len(sizes), seed=5, max_angle=0.02, max_translation=0.05)
    huber = ("huber", synth.REPROJ_HUBER_THRESHOLD)
    out = {}
    for dtype in ("f64", "f32"):
        ndt = [NdtDataset.from_planes(ctx, np.ascontiguousarray(_ndt_planes(1000)[:, :n]), dtype) for n in sizes]
        rep = [ReprojDataset.from_planes(ctx, np.ascontiguousarray(_reproj_planes(1000)[:, 200:200 + n]), dtype) for n in sizes]
        o = out[dtype] = {}
        R, t, reports = api.solve6_batch(ndt, R0, t0, EXP, max_iterations=30)
        o["solve6_batch"] = {"R": R, "t": t, "rows": [_lone((R[i], t[i], rep)) for i, rep in enumerate(reports)]}
        o["solve6_lone"] = [_lone(ds.solve6(R0[i], t0[i], EXP, max_iterations=30)) for i, ds in enumerate(ndt)]
        R, t, reports = api.reproj_solve_batch(rep, R0, t0, synth.REPROJ_INTR4, huber, max_iterations=30)
        o["reproj_batch"] = {"R": R, "t": t, "rows": [_lone((R[i], t[i], rep)) for i, rep in enumerate(reports)]}
        o["reproj_lone"] = [_lone(ds.solve(R0[i], t0[i], synth.REPROJ_INTR4, huber, max_iterations=30)) for i, ds in enumerate(rep)]
        for ds in ndt + rep:
            ds.close()
    return out


def _lone(result):
    """a lone solve; `launches` and `fallback` (see _report) go under "_how": verify reads them, the runs are not compared by them"""
    R, t, rep = result
    return {"R": R, "t": t, "report": _report(rep), "_how": {"launches": rep["launches"], "fallback": rep["fallback"]}}


def _verify_solve_batches(raw):
    """every row is its lone solve, bit for bit, launches included when neither fell back (tests/test_batch_solve.py)"""
    for dtype in ("f64", "f32"):
        for batch, lone in (("solve6_batch", "solve6_lone"), ("reproj_batch", "reproj_lone")):
            for i, (got, row) in enumerate(zip(raw[dtype][batch]["rows"], raw[dtype][lone])):
                assert freeze(got) == freeze(row), (dtype, batch, i, differing(freeze(got), freeze(row)))
                if not (got["_how"]["fallback"] or row["_how"]["fallback"]):
                    assert got["_how"]["launches"] == row["_how"]["launches"], (dtype, batch, i)
            assert any(r["report"]["ok"] for r in raw[dtype][batch]["rows"]), (dtype, batch)


@_case("register_and_score_batches", verify=lambda raw, oracle: _verify_score_batches(raw))
def _run_register_and_score_batches(ctx):
    """register6_batch on a snapshot (an NdtMap); score_batch with scans of 0, 1, C and C + 1 points"""
    from nonlinear_optimizer_for_slam_amd import api
    means, S, valid, _ = _map_inputs()
    gm = api.NdtMap(ctx, means, S, valid, 1.0)
    rng = np.random.default_rng(77)
    C = api.SCORE_CHUNK_POINTS
    clouds = [means[rng.integers(0, len(means), size=n)] + rng.normal(scale=0.5, size=(n, 3)) for n in (0, 1, C, C + 1)]
    scans = [api.Scan(ctx, c) for c in clouds]
    R0, t0 = np.tile(POSE[0].reshape(9), (len(scans), 1)), np.tile(POSE[1], (len(scans), 1))
    out = {"score": [api.score_batch(gm, scans, R0, t0, loss) for loss in NDT_LOSSES],
           "register6": _register_out(api.register6_batch(gm, scans[1:], R0[1:], t0[1:], EXP, keep_multiple=4)),
           "register3": _register_out(api.register3_batch(gm, scans[1:], R0[1:], t0[1:], EXP, keep_multiple=4)),
           "clouds": clouds}
    for h in scans + [gm]:
        h.close()
    return out


def _verify_score_batches(raw):
    means, S, valid, _ = _map_inputs()
    for rows in raw["score"]:
        for row, cloud in zip(rows, raw["clouds"]):
            matches, points = _nearest_two(means, valid, cloud @ POSE[0].T + POSE[1], 1.0) if len(cloud) else (0, 0)
            assert (int(row["matches"]), int(row["matched_points"])) == (matches, points), (len(cloud), row, matches, points)
    assert raw["score"][1][2]["matches"] > 500 and any(r["ok"] for r in raw["register6"]["reports"])


# ------------------------------------------------------------------------------------------------ PlaceDatabase

@_case("place_database", verify=lambda raw, oracle: _verify_place_database(raw))
def _run_place_database(ctx):
    """17 places, by scan and by descriptor, across one doubling of the store; get, and search with 5 queries"""
    from nonlinear_optimizer_for_slam_amd import api
    from tests import place_inputs
    db = api.PlaceDatabase(ctx)
    descs = place_inputs.random_descriptors(17, 20, 60, seed=3)
    out = {"index": []}
    for k in range(17):
        if k % 2:
            sc = api.Scan(ctx, _place_points(k))
            out["index"].append(db.add(sc))
            sc.close()
        else:
            out["index"].append(db.add(descs[k]))
    out["len"] = len(db)
    out["get"] = [db.get(k) for k in range(17)]
    out["search"] = list(db.search(place_inputs.random_descriptors(5, 20, 60, seed=4)))
    out["search_one"] = list(db.search(descs[4], first=2, count=9))
    sc = api.Scan(ctx, _place_points(3))
    out["search_scan"] = list(db.search(sc))
    sc.close()
    db.close()
    return out


@functools.lru_cache(maxsize=None)
def _place_points(k):
    from tests import place_inputs
    return place_inputs.scan_points(600, 20, 60, seed=50 + k)[0]


def _verify_place_database(raw):
    """stored descriptors bit for bit; distances to 1e-12 and shifts where the runner-up is 1e-9 away: tests/test_place_search.py"""
    from tests import place_inputs
    descs = place_inputs.random_descriptors(17, 20, 60, seed=3)
    want = np.stack([place_inputs.descriptor(_place_points(k), 20, 60)[0] if k % 2 else descs[k] for k in range(17)])
    assert raw["index"] == list(range(17)) and raw["len"] == 17
    for k in range(17):
        assert raw["get"][k].tobytes() == want[k].tobytes(), k
    queries = place_inputs.random_descriptors(5, 20, 60, seed=4)
    for q in range(5):
        d, shift, gap = place_inputs.distance(queries[q], want)
        np.testing.assert_allclose(raw["search"][0][q], d, rtol=0, atol=1e-12)
        clear = gap > 1e-9
        assert np.array_equal(raw["search"][1][q][clear], shift[clear]), q
    d, shift, gap = place_inputs.distance(want[3], want)
    np.testing.assert_allclose(raw["search_scan"][0], d, rtol=0, atol=1e-12)
    assert raw["search_scan"][1][3] == 0 and raw["search_scan"][0][3] <= 1e-12


# --------------------------------------------------------------------------------------------------- pose graph

@functools.lru_cache(maxsize=None)
def _pgo_graph():
    """a chain of 13 poses with two loop closures, pose 0 fixed; information matrices for the weighted form"""
    from oracle import oracle_pgo as op
    from tests import pgo_info_inputs
    d = op.with_edges(op.random_graph(13, 0, seed=61), [(1, 8), (4, 12)], seed=62)
    assert d["init"].shape[0] == 13 and d["ref"].size == 14
    return d, pgo_info_inputs.draw_information(14, 63)


PGO_LOSS = ("huber", 0.5)


def _pgo(weighted, block, precond):
    def run(ctx):
        from nonlinear_optimizer_for_slam_amd import pgo
        d, information = _pgo_graph()
        robust = (np.arange(14) >= 12).astype(np.uint8)  # the loss on the two loop closures
        with ctx.options(pgo_block=block, pgo_precond=precond):
            g = pgo.PoseGraph(ctx, d["init"], d["ref"], d["qry"], d["meas"], fixed=d["fixed"],
                              **({"information": information, "loss": PGO_LOSS, "robust": robust} if weighted else {}))
            out = {"n_unknowns": g.n_unknowns, "layout": g.layout_info(), "rounds": []}
            for lam in (1e-3, 6e-4):
                o = {"linearize": list(g.linearize()), "gradient": g.vector("gradient"), "hdiag": g.vector("hdiag"),
                     "weights": g.edge_weights()}
                o["solve"] = list(g.solve(lam, 12, 0.0))  # a fixed iteration count: the tolerance is never met
                o["step"] = g.vector("step")
                g.retract()
                o["state"] = list(g.state())
                out["rounds"].append(o)
            g.close()
        return out

    def verify(raw, oracle):
        from oracle import oracle_pgo as op
        d, _ = _pgo_graph()
        assert raw["rounds"][0]["solve"][0] == 12
        if weighted:  # the float64 restatement of the weighted rule under the loss (tests/pgo_robust_inputs.py)
            from tests import pgo_robust_inputs
            ref = pgo_robust_inputs.RobustGraph(d["init"], d["ref"], d["qry"], d["meas"], _pgo_graph()[1], None, None, d["fixed"],
                                                loss=PGO_LOSS, robust=np.arange(14) >= 12)
            H, g, cost = ref.linearize()
            w, want_w = raw["rounds"][0]["weights"], ref.weights()
            assert np.all(w[:12] == 1.0) and want_w.min() < 0.5  # the loss bites on a loop closure, and only there
            np.testing.assert_allclose(w, want_w, rtol=0, atol=1e-11)  # w <= 1: the gradient's bound below
        else:
            H, g, cost = op.Graph(d["init"], d["ref"], d["qry"], d["meas"], None, None, d["fixed"]).linearize()
        got_cost, gnorm = raw["rounds"][0]["linearize"]  # the bounds of tests/test_pgo.py
        assert abs(got_cost - cost) <= 1e-12 * cost
        np.testing.assert_allclose(raw["rounds"][0]["gradient"], g, rtol=0, atol=1e-11 * np.max(np.abs(g)))
        assert abs(gnorm - np.linalg.norm(g)) <= 1e-12 * np.linalg.norm(g)
        assert raw["rounds"][1]["linearize"][0] < got_cost  # the step went downhill

    return run, verify


for _weighted in (False, True):
    for _block in (0, 1):
        for _precond in (0, 1):
            CASES["pgo_%s_block%d_precond%d" % ("weighted_huber" if _weighted else "plain", _block, _precond)] = _pgo(_weighted, _block, _precond)
