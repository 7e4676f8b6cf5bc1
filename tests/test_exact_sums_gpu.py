"""Every sum path against exact integer sums (tests/exact_inputs.py), at the sizes where a layout, a tail, a pad or the choice
between two forms changes: 0, 1, 2, the wave and block edges, the single-workgroup limit, the default per-pass chunk, the
per-pass grid cap (kMaxPartialRows chunks), the resident capacity of the one-launch solve (capacity + 1 streams), 10 M and
80 M.  The datasets are built so that every per-item term and every partial sum is an integer (or an integer over a power
of two) small enough for the kernel's arithmetic to be exact, in fp32 as in fp64: the GPU's sums must EQUAL the integer
sums, bit for bit.  A correspondence lost or counted twice, a pad that contributes, a stale partial row — any of them
changes the answer, whatever the other paths do.

Every boundary is derived from the library's sources (exact_inputs.library_constants), from the template arguments of the
kernel that ran, and from the device's CU count; each case asserts which kernel or form ran.
"""
import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import Context, NdtDataset, NdtIndexedDataset, ReprojDataset
from tests import exact_inputs as X

pytestmark = pytest.mark.gpu

T_NAME = {"f64": "double", "f32": "float"}
ES = {"f64": 8, "f32": 4}
K = X.library_constants()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _eq(got, want, what):
    got = np.asarray(got, dtype=np.float64)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d sums differ, first at %d: %r != %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def _geometry(ctx, dtype, reproj=False):
    """Template arguments of the default per-pass kernel (probed on a one-item dataset)."""
    cls, planes = (ReprojDataset, np.ones((5, 1))) if reproj else (NdtDataset, np.zeros((15, 1)))
    ds = cls.from_planes(ctx, planes, dtype)
    if reproj:
        ds.accumulate(np.eye(3), np.zeros(3), X.REPROJ_INTR, None, X.REPROJ_MIN_DEPTH)
    else:
        ds.accumulate6(np.eye(3), np.zeros(3))
    ds.close()
    return X.assemble_geometry(ctx.last_kernel())


def solve_form(n, planes, dtype, cus):
    return X.solve_items_per_lane(n, planes, ES[dtype], K, cus)[0]


def _check_form(ctx, problem, n, planes, dtype, cus, budget=None):
    """The form that ran is the one solve_items_per_lane predicts, and its lanes stay within the dataset's budget."""
    name = ctx.last_kernel()
    form, per_lane = X.solve_items_per_lane(n, planes, ES[dtype], K, cus)
    assert budget is None or per_lane <= budget, (n, form, per_lane, budget)
    if form == "single":
        assert "solve_single_block_kernel<nos::%s<%s" % (problem, T_NAME[dtype]) in name, (n, name)
        return form
    g = X.cluster_geometry(name)
    assert g["problem"] == problem and g["T"] == T_NAME[dtype], (n, name)
    if form == "resident":
        assert g["SI"] == 0 and g["RI"] + g["LI"] == K["resident"][(planes, ES[dtype])], (n, name)
    else:
        assert g["SI"] == K["stream_items"][ES[dtype]] and g["RI"] == g["LI"] == 0, (n, name)
    return form


def resident_plus_one(dtype, cus, planes=15):
    """The first size the resident one-launch solve cannot hold: it streams."""
    return K["resident"][(planes, ES[dtype])] * 512 * min(K["cluster_max_blocks"], cus) + 1


def ndt_sizes(dtype, geom, cus):
    single = K["single_block_max_elements"] // 15
    chunk = geom["BLOCK"] * geom["ITEMS"]
    resident = resident_plus_one(dtype, cus) - 1
    rows = K["max_partial_rows"] * chunk
    sizes = {0, 1, 2, 63, 64, 65, 255, 256, 257, single - 1, single, single + 1, chunk - 1, chunk, chunk + 1,
             resident - 1, resident, resident + 1, rows - 1, rows, rows + 1}
    return sorted(sizes)


def _ndt_paths(ctx, ds, case, n, dtype, cus, geom, losses):
    """accumulate6 / accumulate3 and the first cost of solve6 / solve3 of one dataset against the exact sums."""
    T = T_NAME[dtype]
    for loss in losses:
        what = "n=%d %s %s" % (n, dtype, loss and loss[0])
        _eq(ds.accumulate6(case.R, case.t, loss), case.want6, "accumulate6 " + what)
        g = X.assemble_geometry(ctx.last_kernel())
        assert g["problem"] == "Ndt6Problem" and g["T"] == T and (g["ITEMS"], g["BLOCK"]) == (geom["ITEMS"], geom["BLOCK"])
        _eq(ds.accumulate3(case.R2, case.t2, loss), case.want3, "accumulate3 " + what)
        assert "assemble_kernel<nos::Ndt3Problem<%s" % T in ctx.last_kernel()
        _, _, rep = ds.solve6(case.R, case.t, loss, max_iterations=1)
        form = _check_form(ctx, "Ndt6Problem", n, 15, dtype, cus, case.lane_budget)
        assert rep["launches"] == 1
        _eq(rep["cost_history"][:1], case.want6[27:], "%s solve6 first cost %s" % (form, what))
        _, _, rep = ds.solve3(case.R2, case.t2, loss, max_iterations=1)
        form = _check_form(ctx, "Ndt3Problem", n, 15, dtype, cus, case.lane_budget)
        _eq(rep["cost_history"][:1], case.want3[9:], "%s solve3 first cost %s" % (form, what))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ndt_sums_are_exact_at_every_boundary(ctx, cus, dtype):
    """Per-pass accumulate6 / accumulate3 and the three solve forms (first cost), no loss and an all-inlier Huber loss,
    at every boundary size below 10 M; the async torch-tensor results and two shards on one device at the chunk edges."""
    import torch
    geom = _geometry(ctx, dtype)
    assert geom["T"] == T_NAME[dtype]
    chunk = geom["BLOCK"] * geom["ITEMS"]
    forms = set()
    for n in ndt_sizes(dtype, geom, cus):
        case = X.ndt_case(n, dtype, cus=cus, seed=n % 1000 + 1)
        # the budget assumes at least one wave per CU; the per-pass launch gives each lane far fewer items
        assert X.pass_items_per_lane(n, geom, K, cus) <= case.lane_budget
        ds = NdtDataset.from_planes(ctx, case.planes, dtype)
        _ndt_paths(ctx, ds, case, n, dtype, cus, geom, (None, case.huber))
        forms.add(solve_form(n, 15, dtype, cus))
        if n in (1, chunk - 1, chunk + 1, 257):
            out6 = torch.zeros(28, dtype=torch.float64, device="cuda")
            out3 = torch.zeros(10, dtype=torch.float64, device="cuda")
            ctx.use_torch_stream()
            ds.accumulate6_async(case.R, case.t, None, out6)
            ds.accumulate3_async(case.R2, case.t2, None, out3)
            torch.cuda.synchronize()
            ctx.set_stream(0)
            _eq(out6.cpu().numpy(), case.want6, "async accumulate6 n=%d %s" % (n, dtype))
            _eq(out3.cpu().numpy(), case.want3, "async accumulate3 n=%d %s" % (n, dtype))
        ds.close()
        if n in (2, chunk - 1, chunk + 1, resident_plus_one(dtype, cus)):
            c2 = Context((0, 0))
            sh = NdtDataset.from_planes(c2, case.planes, dtype)
            _eq(sh.accumulate6(case.R, case.t, case.huber), case.want6, "2 shards accumulate6 n=%d %s" % (n, dtype))
            assert "assemble_kernel<nos::Ndt6Problem<%s" % T_NAME[dtype] in c2.last_kernel(1)
            _eq(sh.accumulate3(case.R2, case.t2), case.want3, "2 shards accumulate3 n=%d %s" % (n, dtype))
            sh.close()
            c2.close()
    assert forms == {"single", "resident", "streamed"}, forms


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_indexed_sums_are_exact(ctx, cus, dtype):
    """NdtIndexedDataset: one voxel per point in a shuffled table, a second slot on every fifth point (−1 elsewhere);
    accumulate6 / accumulate3 and the first cost of its solve against the exact sums over the (point, voxel) pairs."""
    single = K["single_block_max_elements"] // 15
    for n in (1, 65, single + 1, 100_003):
        case = X.ndt_case(n, dtype, cus=cus, seed=n % 1000 + 7, three=False)
        rng = np.random.default_rng(n)
        order = rng.permutation(n)  # voxel v of the table holds the (mu, S) of point order[v]
        slot0 = np.empty(n, dtype=np.int32)
        slot0[order] = np.arange(n, dtype=np.int32)
        slot1 = np.full(n, -1, dtype=np.int32)
        extra = np.arange(0, n, 5)
        slot1[extra] = slot0[(extra + 1) % n]
        pairs = np.concatenate([case.planes, case.planes[:, extra]], axis=1)
        pairs[3:15, n:] = case.planes[3:15, (extra + 1) % n]
        want6, want3 = X.ndt_sums_of_planes(pairs, case.R, case.t, case.R2, case.t2, dtype, cus)
        means = case.planes[3:6, order].T
        S = case.planes[6:15, order].T.reshape(-1, 3, 3)
        ids = NdtIndexedDataset.from_arrays(ctx, case.planes[0:3].copy(), np.stack([slot0, slot1]), means, S, dtype)
        _eq(ids.accumulate6(case.R, case.t), want6, "indexed accumulate6 n=%d %s" % (n, dtype))
        _eq(ids.accumulate3(case.R2, case.t2), want3, "indexed accumulate3 n=%d %s" % (n, dtype))
        _, _, rep = ids.solve6(case.R, case.t, None, max_iterations=1)
        _eq(rep["cost_history"][:1], want6[27:], "indexed solve6 first cost n=%d %s" % (n, dtype))
        ids.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ndt_sums_are_exact_at_ten_million(ctx, cus, dtype):
    """BASELINE.json configs[1]'s size: per-pass accumulate6 / accumulate3 and the streamed one-launch solve."""
    n = 10_000_000
    geom = _geometry(ctx, dtype)
    case = X.ndt_case(n, dtype, cus=cus, seed=10)
    assert X.pass_items_per_lane(n, geom, K, cus) <= case.lane_budget
    assert solve_form(n, 15, dtype, cus) == "streamed"
    ds = NdtDataset.from_planes(ctx, case.planes, dtype)
    _ndt_paths(ctx, ds, case, n, dtype, cus, geom, (case.huber,))
    ds.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_ndt_sums_are_exact_at_eighty_million(ctx, cus, dtype):
    """BASELINE.json configs[3]'s size on one device: per-pass accumulate6 and the streamed one-launch solve's first
    cost.  fp32 lanes sum ≈ 600 items each in fp32 here; the integers keep every partial below 2^24."""
    n = 80_000_000
    geom = _geometry(ctx, dtype)
    case = X.ndt_case(n, dtype, cus=cus, seed=80, three=False)
    assert X.pass_items_per_lane(n, geom, K, cus) <= case.lane_budget
    ds = NdtDataset.from_planes(ctx, case.planes, dtype)
    del case.planes
    assert len(ds) == n
    _eq(ds.accumulate6(case.R, case.t, case.huber), case.want6, "accumulate6 n=%d %s" % (n, dtype))
    assert X.assemble_geometry(ctx.last_kernel())["problem"] == "Ndt6Problem"
    _, _, rep = ds.solve6(case.R, case.t, None, max_iterations=1)
    assert _check_form(ctx, "Ndt6Problem", n, 15, dtype, cus) == "streamed"
    _eq(rep["cost_history"][:1], case.want6[27:], "streamed solve6 first cost n=%d %s" % (n, dtype))
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reprojection_sums_are_exact_at_every_boundary(ctx, cus, dtype):
    """Reprojection accumulate (per pass, ping-pong kernel) and solve (first cost) with depths a power of two: fast_inv
    returns 1/z exactly, so the sums are exact; items at depth 0 or −z must not count.  Sizes: the wave / block edges,
    the single-workgroup limit (3 072 correspondences of 5 planes), the per-pass chunk and the resident capacity ± 1."""
    import torch
    geom = _geometry(ctx, dtype, reproj=True)
    assert geom["problem"] == "ReprojProblem" and geom["PREFETCH"] == 3
    chunk = geom["BLOCK"] * geom["ITEMS"]
    single = K["single_block_max_elements"] // 5
    resident = K["resident"][(5, ES[dtype])] * 512 * min(K["cluster_max_blocks"], cus)
    forms = set()
    for n in sorted({1, 2, 63, 64, 65, 255, 256, 257, single - 1, single, single + 1, chunk - 1, chunk + 1, 2 * chunk + 1,
                     resident - 1, resident, resident + 1, 10_000_000}):
        case = X.reproj_case(n, dtype, cus=cus, seed=n % 1000 + 3)
        assert X.pass_items_per_lane(n, geom, K, cus) <= case.lane_budget
        ds = ReprojDataset.from_planes(ctx, case.planes, dtype)
        for loss in (None, case.huber):
            what = "n=%d %s %s" % (n, dtype, loss and loss[0])
            _eq(ds.accumulate(case.R, case.t, X.REPROJ_INTR, loss, X.REPROJ_MIN_DEPTH), case.want, "reprojection accumulate " + what)
            assert "assemble_kernel<nos::ReprojProblem<%s" % T_NAME[dtype] in ctx.last_kernel()
            _, _, rep = ds.solve(case.R, case.t, X.REPROJ_INTR, loss, X.REPROJ_MIN_DEPTH, max_iterations=1)
            form = _check_form(ctx, "ReprojProblem", n, 5, dtype, cus, case.lane_budget)
            forms.add(form)
            _eq(rep["cost_history"][:1], case.want[27:], "reprojection %s solve first cost %s" % (form, what))
        if n in (1, chunk + 1):
            out = torch.zeros(28, dtype=torch.float64, device="cuda")
            ctx.use_torch_stream()
            ds.accumulate_async(case.R, case.t, X.REPROJ_INTR, None, out, X.REPROJ_MIN_DEPTH)
            torch.cuda.synchronize()
            ctx.set_stream(0)
            _eq(out.cpu().numpy(), case.want, "reprojection async accumulate n=%d %s" % (n, dtype))
        ds.close()
    assert forms == {"single", "resident", "streamed"}, forms
