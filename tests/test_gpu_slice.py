"""The device slicer (csrc/psg_slice.hip, harness.ScannetDatasetWholeScene.device_item, slicer="device")
on the MI355X: the kernels against tests/slice_ref.py, device_item against __getitem__ and the reference's recorded blocks,
and the two evaluation loops with slicer="device" against slicer="host".  Everything bit for bit; no tolerance anywhere."""
import numpy as np
import pytest
import torch

import slice_ref
from test_gpu_harness import synth_scene
from test_slice_host import GOLDEN, assert_same, fixture_dataset, same_state

pytestmark = pytest.mark.gpu
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)      # lanes, waves, the 256-point tile, the 1024-point workgroup


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def crafted():
    return slice_ref.crafted_scenes()


@pytest.fixture(scope="module")
def net(weights_sd):
    from pointsecguard_amd.models.pointnet2_sem_seg import get_model
    m = get_model(13).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights_sd.items()})
    return m


def two_scene_dataset():
    from pointsecguard_amd import harness
    scenes = {"Area_5_a.npy": synth_scene(11, 5000, 1.6, 1.2), "Area_5_b.npy": synth_scene(12, 3000, 1.0, 1.4)}
    return harness.ScannetDatasetWholeScene(None, block_points=1024, scenes=scenes)


def to_host(item):
    return tuple(t.cpu().numpy() for t in item)


def device_lists(rows, windows):
    """psg_slice_count + psg_slice_members on rows [n, k] float64 (x, y = the first two columns) -> counts, cell_off, inside"""
    from pointsecguard_amd import _lib, runtime
    dev = torch.device("cuda")
    pts = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    win = torch.from_numpy(np.ascontiguousarray(windows)).to(dev)
    n, n_cells = rows.shape[0], windows.shape[0]
    items = n_cells * (-(-n // _lib.SLICE_TILE)) + 1
    tile_off = torch.empty(items, dtype=torch.int32, device=dev)
    counts = torch.full((n_cells,), -7, dtype=torch.int32, device=dev)
    cell_off = torch.full((n_cells + 1,), -7, dtype=torch.int32, device=dev)
    _lib.call("psg_slice_count", runtime.ptr(pts), rows.shape[1], n, runtime.ptr(win), n_cells, runtime.ptr(tile_off), items,
              runtime.ptr(counts), runtime.ptr(cell_off), runtime.stream())
    total = int(counts.cpu().numpy().astype(np.int64).sum())
    inside = torch.full((total + 3,), -7, dtype=torch.int32, device=dev)          # (three guard words behind the lists)
    if total:
        _lib.call("psg_slice_members", runtime.ptr(pts), rows.shape[1], n, runtime.ptr(win), n_cells, runtime.ptr(tile_off), items,
                  runtime.ptr(inside), total, runtime.stream())
    inside = inside.cpu().numpy()
    assert (inside[total:] == -7).all()
    return counts.cpu().numpy(), cell_off.cpu().numpy(), inside[:total]


def check_lists(rows, windows, what):
    counts, cell_off, inside = device_lists(rows, windows)
    want_inside, want_off = slice_ref.members(rows[:, 0], rows[:, 1], windows)
    assert np.array_equal(counts, slice_ref.count(rows[:, 0], rows[:, 1], windows)), what
    assert np.array_equal(cell_off, want_off), what
    assert np.array_equal(inside, want_inside), what
    return counts


def scene_windows(ds, si):
    pts = ds.scene_points_list[si]
    return slice_ref.cells(np.amin(pts, axis=0)[:3], np.amax(pts, axis=0)[:3], ds.block_size, ds.stride, ds.padding)[0]


# ------------------------------------------------------------------------------------------------- the kernels alone
def test_lists_of_the_fixture_and_crafted_scenes(g, crafted):
    fx = fixture_dataset(g)
    for si in range(len(fx)):
        check_lists(fx.scene_points_list[si], scene_windows(fx, si), "fixture %d" % si)
    for name, room in crafted.items():
        ds = slice_ref.dataset(room)
        counts = check_lists(ds.scene_points_list[0], scene_windows(ds, 0), name)
        if name == "hole":
            assert counts[1] == 0
        if name == "exact_multiple":
            assert counts.tolist() == [128]                     # a one-cell grid


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_lists_at_the_compaction_edges(n):
    rng = np.random.default_rng(n)
    windows = slice_ref.cells((0.0, 0.0, 0.0), (2.0, 1.0, 2.8), 1.0, 0.5, 0.001)[0]
    rows = np.stack((rng.random(n) * 2.0, rng.random(n)), axis=1)
    # a member of all three cells in the first and the last lane of the first and the last wave, tile and workgroup
    for k in (0, 63, 64, 255, 256, 1023, 1024, n - 64, n - 1):
        if 0 <= k < n:
            rows[k] = (1.0, 0.5)
    counts = check_lists(rows, windows, "n = %d, stride 2" % n)
    assert (counts >= 1).all()
    wide = np.concatenate((rows, rng.random((n, 4))), axis=1)
    check_lists(wide, windows, "n = %d, stride 6" % n)
    check_lists(rows, windows[1:2], "n = %d, one cell" % n)


def test_two_runs_give_the_same_lists(crafted):
    room = crafted["n4097"]
    ds = slice_ref.dataset(room)
    a = device_lists(ds.scene_points_list[0], scene_windows(ds, 0))
    b = device_lists(ds.scene_points_list[0], scene_windows(ds, 0))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------- device_item
def item_pair(ds, si, seed):
    """(device_item, its generator state, __getitem__ after the harness's casts, its state) under the same seed"""
    np.random.seed(seed)
    dev_item = to_host(ds.device_item(si))
    dev_state = np.random.get_state()
    np.random.seed(seed)
    host = slice_ref.host_item(ds, si)
    return dev_item, dev_state, host, np.random.get_state()


def test_device_item_on_the_reference_fixture(g):
    ds = fixture_dataset(g)
    for si in range(len(ds)):
        before = ds.scene_points_list[si].copy()
        got, state, host, host_state = item_pair(ds, si, 100 + si)
        want = (g["data_room%d" % si].astype(np.float32), g["label_room%d" % si].astype(np.int32),
                g["sample_weight%d" % si].astype(np.float32), g["index_room%d" % si].astype(np.int32))
        assert_same(got, want, "reference, scene %d" % si)
        assert_same(got, host, "__getitem__, scene %d" % si)
        assert same_state(state, host_state)
        assert np.array_equal(ds.scene_points_list[si], before)


def test_device_item_on_the_crafted_scenes(crafted):
    for name, room in crafted.items():
        ds = slice_ref.dataset(room)
        got, state, host, host_state = item_pair(ds, 0, 7)
        assert_same(got, host, name)
        assert same_state(state, host_state), name


def test_device_item_on_the_two_scene_dataset():
    ds = two_scene_dataset()
    before = [a.copy() for a in ds.scene_points_list]
    for si in range(2):
        got, state, host, host_state = item_pair(ds, si, 3)
        assert got[0].shape[1:] == (1024, 9)
        assert_same(got, host, "scene %d" % si)
        assert same_state(state, host_state)
    assert all(np.array_equal(a, b) for a, b in zip(ds.scene_points_list, before))


def test_reproducibility():
    ds = two_scene_dataset()
    np.random.seed(3)
    first, second = to_host(ds.device_item(0)), to_host(ds.device_item(0))      # two calls in a row, one seed
    np.random.seed(3)
    again = to_host(ds.device_item(0))
    assert_same(again, first, "same seed")
    np.random.seed(3)
    host_first, host_second = slice_ref.host_item(ds, 0), slice_ref.host_item(ds, 0)
    assert_same(first, host_first, "first call")
    assert_same(second, host_second, "second call")
    assert not np.array_equal(first[3], second[3])


def test_moved_scene():
    """xyz=: the scene with other coordinates - here pushed out so that the corners, and with them the grid, change"""
    from pointsecguard_amd import harness
    room = synth_scene(11, 5000, 1.6, 1.2)
    rng = np.random.default_rng(5)
    moved = room[:, :3] + rng.normal(0.0, 0.02, (5000, 3))
    moved[np.argmax(moved[:, 0]), 0] += 0.5
    moved_room = room.copy()
    moved_room[:, :3] = moved
    ds = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": room})
    ds_moved = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": moved_room})
    grid = lambda r: slice_ref.cells(r[:, :3].min(axis=0), r[:, :3].max(axis=0), 1.0, 0.5, 0.001)[2]
    assert grid(room) != grid(moved_room)
    np.random.seed(3)
    want = slice_ref.host_item(ds_moved, 0)
    want_state = np.random.get_state()
    for form in (moved, torch.from_numpy(moved).cuda()):
        np.random.seed(3)
        got = to_host(ds.device_item(0, xyz=form))
        assert_same(got, want, type(form).__name__)
        assert same_state(np.random.get_state(), want_state)
    got, _, host, _ = item_pair(ds, 0, 3)
    assert_same(got, host, "the scene itself, afterwards")
    with pytest.raises(ValueError):
        ds.device_item(0, xyz=moved.astype(np.float32))
    with pytest.raises(ValueError):
        ds.device_item(0, xyz=moved[:-1])


# ------------------------------------------------------------------------------------------------- the evaluation loops
def both_slicers(tmp_path, call):
    """call(slicer, log_path) under the same seeds -> the two result dicts; asserts equal results, logs and generator states"""
    out = {}
    for slicer in ("host", "device"):
        np.random.seed(3)
        torch.manual_seed(3)
        path = tmp_path / ("%s.txt" % slicer)
        res = call(slicer, str(path))
        torch.cuda.synchronize()
        out[slicer] = (res, path.read_bytes(), np.random.get_state(), torch.get_rng_state())
    (rh, lh, nh, th), (rd, ld, nd, td) = out["host"], out["device"]
    assert np.array_equal(rh["counters"], rd["counters"]) and rh["scenes"] == rd["scenes"]
    assert {k: v for k, v in rh.items() if k != "counters"} == {k: v for k, v in rd.items() if k != "counters"}
    assert lh == ld and len(lh.splitlines()) > 1
    assert same_state(nh, nd) and torch.equal(th, td)
    return rh, rd


@pytest.mark.parametrize("streams", (1, 3))
def test_whole_scene_loop(tmp_path, net, streams):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks import torchattacks
    ds = two_scene_dataset()
    both_slicers(tmp_path, lambda slicer, path: harness.evaluate_whole_scene(
        net, ds, lambda m: torchattacks.NB_attack(m, eps=0.1, alpha=0.05, iters=2), batch_size=4, streams=streams, log_path=path,
        log=lambda *_: None, slicer=slicer))


def test_whole_scene_loop_targeted(tmp_path, net):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks import torchattacks
    ds = two_scene_dataset()
    origin = int(np.bincount(ds.semantic_labels_list[0].astype(np.int64)).argmax())        # the scene's most frequent label
    target = (origin + 1) % 13
    both_slicers(tmp_path, lambda slicer, path: harness.evaluate_whole_scene(
        net, ds, lambda m, t, mask: torchattacks.tar_NB_attack(m, eps=0.1, alpha=0.05, iters=2, target=t, mask=mask), batch_size=4, streams=1,
        log_path=path, log=lambda *_: None, targeted=dict(origin=origin, target=target), slicer=slicer))


def test_consistent_loop(tmp_path, net):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    ds = two_scene_dataset()
    both_slicers(tmp_path, lambda slicer, path: harness.evaluate_whole_scene_consistent(
        net, ds, lambda m: SceneNBAttack(m, 0.1, 0.05, 2), batch_size=4, log_path=path, log=lambda *_: None, slicer=slicer))


def test_consistent_loop_targeted(tmp_path, net):
    from pointsecguard_amd import harness
    from pointsecguard_amd.attacks.scene import SceneNBAttack
    ds = two_scene_dataset()
    origin = int(np.bincount(ds.semantic_labels_list[0].astype(np.int64)).argmax())
    target = (origin + 1) % 13
    both_slicers(tmp_path, lambda slicer, path: harness.evaluate_whole_scene_consistent(
        net, ds, lambda m: SceneNBAttack(m, 0.5, 0.1, 2, target=target, origin=origin), batch_size=4, log_path=path,
        log=lambda *_: None, targeted=dict(origin=origin, target=target), slicer=slicer))


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals(net):
    from pointsecguard_amd import harness
    room = synth_scene(11, 5000, 1.6, 1.2)
    f32 = harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": room.astype(np.float32)})
    with pytest.raises(ValueError, match='slicer="host"'):
        f32.device_item(0)
    bad = room.copy()
    bad[5, 6] = 13.0
    with pytest.raises(IndexError):
        harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": bad}).device_item(0)
    fine = harness.ScannetDatasetWholeScene(None, block_points=1024, stride=0.01, scenes={"Area_5_a.npy": room})
    gx, gy = slice_ref.cells(room[:, :3].min(axis=0), room[:, :3].max(axis=0), 1.0, 0.01, 0.001)[2]
    assert gx * gy > 1024 >= gx and 1024 >= gy                     # over the cap by the product, not by one axis
    state = np.random.get_state()
    with pytest.raises(ValueError, match='slicer="host"'):
        fine.device_item(0)
    assert same_state(state, np.random.get_state())               # refused before a draw

    class HostOnly:
        """a caller's dataset class: sliced in line by the host path, no device_item"""
        def __init__(self, ds):
            self.ds, self.block_points = ds, ds.block_points
            self.semantic_labels_list, self.file_list = ds.semantic_labels_list, ds.file_list

        def __len__(self):
            return len(self.ds)

        def __getitem__(self, i):
            return self.ds[i]
    ds = HostOnly(harness.ScannetDatasetWholeScene(None, block_points=1024, scenes={"Area_5_a.npy": room}))
    with pytest.raises(TypeError, match="device_item"):
        harness.evaluate_whole_scene(net, ds, None, slicer="device", log=lambda *_: None)
    with pytest.raises(ValueError, match="slicer"):
        harness.evaluate_whole_scene(net, ds, None, slicer="gpu", log=lambda *_: None)
