"""The host-resident ImageNet set without a device: the loader's memory accounting, the flag, the dataset against
the resident one, the two-half prefetch protocol over a recording stand-in for the stager, the CPU index stream and
its resume, and the gather threads' shutdown."""
import json
import threading

import numpy as np
import pytest
import torch

from distributedtf_amd.data import datasets
from distributedtf_amd.data.datasets import (DeviceDataset, HostFeed, HostImageNetDataset, IndexBatch, RowStager,
                                             load_imagenet_arrays)
from distributedtf_amd.utils.flags import parse_main_args


def _write(d, n=40, nv=4, s=8):
    rng = np.random.default_rng(0)
    arrs = {"train_images": rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8),
            "train_labels": rng.integers(0, 5, (n,), dtype=np.int64),
            "val_images": rng.integers(0, 256, (nv, s, s, 3), dtype=np.uint8),
            "val_labels": rng.integers(0, 5, (nv,), dtype=np.int64)}
    for k, v in arrs.items():
        np.save(str(d / (k + ".npy")), v)
    return arrs


def _hp(bs=4):
    return {"opt_case": {"optimizer": "Momentum", "lr": 0.01, "momentum": 0.9}, "batch_size": bs,
            "regularizer": "l2_regularizer", "weight_decay": 1e-4, "initializer": "he_init", "decay_steps": 0,
            "decay_rate": 1.0}


def _model(tmp_path, cid=0, seed=1, **kw):
    from distributedtf_amd.models.imagenet_model import ImageNetModel
    return ImageNetModel(cid, _hp(), str(tmp_path / "save" / "model_"), seed=seed, resnet_size=50, image_size=32,
                         device="cpu", backend="torch", checkpoint_every_round=False, capacity=1, **kw)


@pytest.fixture
def fresh_engines():
    from distributedtf_amd.models.engine_model import EngineModel
    EngineModel.reset_engines()
    yield
    EngineModel.reset_engines()


# ------------------------------------------------------------------------------------------------------ loader
def test_loader_counts_staging_not_training_images(tmp_path):
    """40 training and 4 validation images at 8 x 8, staging for 3 rows per half: the resident need counts the
    training images, the host need counts 2 * 3 * 192 bytes of staging in their place."""
    _write(tmp_path)
    common = 4 * 192 + 8 * 44 + 4 * 4 * 192  # validation images, int64 labels, the fp32 evaluation cache
    resident, host = common + 40 * 192, common + 2 * 3 * 192
    assert host < resident
    between = (host + resident) // 2
    with pytest.raises(MemoryError, match="GB"):
        load_imagenet_arrays(str(tmp_path), max_bytes=between)
    with pytest.raises(MemoryError):
        load_imagenet_arrays(str(tmp_path), max_bytes=between, resident=True, stage_rows=3)
    trx, tr_y, vax, va_y = load_imagenet_arrays(str(tmp_path), max_bytes=between, resident=False, stage_rows=3)
    assert isinstance(trx, np.memmap) and trx.shape == (40, 8, 8, 3)
    load_imagenet_arrays(str(tmp_path), max_bytes=host, resident=False, stage_rows=3)  # exactly enough
    with pytest.raises(MemoryError, match="staging"):
        load_imagenet_arrays(str(tmp_path), max_bytes=host - 1, resident=False, stage_rows=3)
    # the resident path is untouched by the keyword: its need and its text
    load_imagenet_arrays(str(tmp_path), max_bytes=resident)
    with pytest.raises(MemoryError, match="store the images at a smaller side"):
        load_imagenet_arrays(str(tmp_path), max_bytes=resident - 1)


# ------------------------------------------------------------------------------------------------------- flags
def test_flag_parses_and_reaches_the_dataset(tmp_path, fresh_engines, capsys):
    a = parse_main_args(["2", "--model", "imagenet", "--imagenet_data", "host", "--use_synthetic_data", "learnable"])
    assert a.imagenet_data == "host" and a.model_kwargs()["imagenet_data"] == "host"
    d = parse_main_args(["2", "--model", "imagenet", "--use_synthetic_data", "learnable"])
    assert d.imagenet_data == "device" and "imagenet_data" not in d.model_kwargs()
    assert parse_main_args(["2"]).imagenet_data == "device"
    for bad in (["--model", "cifar10", "--imagenet_data", "host"],
                ["--model", "imagenet", "--imagenet_data", "host"],  # the fixed synthetic batch: no rows
                ["--model", "imagenet", "--imagenet_data", "host", "--data_dir", str(tmp_path)],  # no arrays there
                ["--model", "imagenet", "--imagenet_data", "disk"]):
        with pytest.raises(SystemExit):
            parse_main_args(["2"] + bad)
        assert "--imagenet_data" in capsys.readouterr().err
    arrays = tmp_path / "data"
    arrays.mkdir()
    _write(arrays)
    assert parse_main_args(["2", "--model", "imagenet", "--imagenet_data", "host", "--data_dir",
                            str(arrays)]).imagenet_data == "host"
    m = _model(tmp_path, use_synthetic_data="learnable", imagenet_data=a.model_kwargs()["imagenet_data"])
    ds = m.make_dataset("cpu")
    assert isinstance(ds, HostImageNetDataset) and isinstance(ds.train_x, np.ndarray) and ds.imagenet
    assert not ds.hip_augment and ds.out_size == 32 and ds.train_y.dtype == torch.int64
    assert m.dataset() is m.dataset() and isinstance(m.dataset(), HostImageNetDataset)
    m.release()
    r = _model(tmp_path, cid=1, data_dir=str(arrays), imagenet_data="host")
    rd = r.make_dataset("cpu")
    assert isinstance(rd, HostImageNetDataset) and isinstance(rd.train_x, np.memmap) and rd.num_train == 40
    r.release()
    from distributedtf_amd.models.engine_model import EngineModel
    for kw, want in ((dict(use_synthetic_data="learnable"), DeviceDataset), (dict(imagenet_data="host"), None)):
        EngineModel.reset_engines()  # (another class count is another engine)
        d = _model(tmp_path, cid=2, **kw)
        if want is None:  # the fixed synthetic batch has no rows to stage
            with pytest.raises(ValueError, match="host"):
                d.make_dataset("cpu")
        else:
            assert type(d.make_dataset("cpu")) is want


# -------------------------------------------------------------------------------------------- dataset equality
def test_host_batch_is_bitwise_the_resident_batch(tmp_path):
    a = _write(tmp_path, n=23, s=40)
    trx = np.load(str(tmp_path / "train_images.npy"), mmap_mode="r")
    kw = dict(out_size=32, seed=21)
    host = HostImageNetDataset(trx, a["train_labels"], a["val_images"], a["val_labels"], "cpu", **kw)
    dev = DeviceDataset(a["train_images"], a["train_labels"], a["val_images"], a["val_labels"], "cpu",
                        augment=datasets.augment_imagenet, eval_transform=datasets.eval_imagenet, **kw)
    for idx in (torch.tensor([22, 0, 7, 7, 3]), torch.tensor([5])):
        hx, hy = host.batch(idx)
        dx, dy = dev.batch(idx)
        assert host.rng_counter == dev.rng_counter and hx.dtype == torch.float32
        assert torch.equal(hx.view(torch.int32), dx.view(torch.int32)) and torch.equal(hy, dy)
    assert host.train_x is trx and isinstance(host.train_x, np.memmap)
    assert host.num_train == 23 and host.device.type == "cpu"
    ex, ey = host.eval_set()
    assert torch.equal(ex, dev.eval_set()[0]) and torch.equal(ey, dev.eval_set()[1])
    with pytest.raises(ValueError):
        HostImageNetDataset(torch.from_numpy(a["train_images"]), a["train_labels"], a["val_images"], a["val_labels"],
                            "cpu", out_size=32)


# ------------------------------------------------------------------------------------------- prefetch protocol
class StubStager:
    """Records what HostFeed asks of a stager and keeps the rows each half would hold.  ``busy``: a step took the
    half (wait_copied) and has not marked it consumed yet -- staging into it then would overwrite rows in use."""

    def __init__(self, cap=0):
        self.cap, self.generation = cap, 0
        self.rows = [None, None]
        self.busy = [False, False]
        self.log = []

    def ensure(self, cap):
        if cap > self.cap:
            assert not any(self.busy)
            self.cap, self.generation, self.rows = cap, self.generation + 1, [None, None]
            self.log.append(("grow", cap))

    def stage(self, rows, half):
        assert not self.busy[half], "half %d restaged before its consumed mark" % half
        assert len(rows) <= self.cap
        self.rows[half] = np.array(rows)
        self.log.append(("stage", half, len(rows)))

    def wait_copied(self, half):
        self.busy[half] = True
        self.log.append(("wait", half))

    def mark_consumed(self, half):
        assert self.busy[half]
        self.busy[half] = False
        self.log.append(("consumed", half))


def test_prefetch_protocol():
    st = StubStager()
    feed = HostFeed(st)
    perm = np.random.default_rng(3).permutation(100)

    def step(rows, announced):
        before = len(st.log)
        half = feed.begin(rows)
        assert np.array_equal(st.rows[half], rows)  # the half the step reads holds the rows it asked for
        assert half == feed.half and st.busy[half] and not st.busy[1 - half]
        feed.end(announced)
        assert not any(st.busy)
        return half, st.log[before:]

    # step 1: nothing staged yet -> synchronous; announces step 2 rightly
    h1, log = step(perm[0:6], perm[6:12])
    assert log == [("grow", 6), ("stage", h1, 6), ("wait", h1), ("consumed", h1), ("stage", 1 - h1, 6)]
    assert (feed.hits, feed.syncs) == (0, 1)
    # step 2: announcement right -> no stage before the wait; announces batch 6, but 10 will be requested
    h2, log = step(perm[6:12], perm[12:18])
    assert h2 == 1 - h1 and log == [("wait", h2), ("consumed", h2), ("stage", h1, 6)]
    assert (feed.hits, feed.syncs) == (1, 1)
    # step 3: announcement wrong (6 announced, 10 requested; the halves grow) -> synchronous; announces rightly
    h3, log = step(perm[12:22], perm[22:32])
    assert h3 == 1 - h2 and log == [("grow", 10), ("stage", h3, 10), ("wait", h3), ("consumed", h3),
                                    ("stage", h2, 10)]
    assert (feed.hits, feed.syncs) == (1, 2)
    # step 4: right again; epoch wrap next: nothing announced
    h4, log = step(perm[22:32], None)
    assert log == [("wait", h4), ("consumed", h4)] and (feed.hits, feed.syncs) == (2, 2)
    # step 5: after the wrap nothing was staged ahead -> synchronous; announces rows of this member set
    perm2 = np.random.default_rng(4).permutation(100)
    h5, log = step(perm2[0:10], perm2[10:20])
    assert h5 == 1 - h4 and log[0] == ("stage", h5, 10) and (feed.hits, feed.syncs) == (2, 3)
    # step 6: the member set changed: same count, other rows than announced -> synchronous
    other = np.concatenate([perm2[10:15], perm[50:55]])
    h6, log = step(other, None)
    assert log[:2] == [("stage", h6, 10), ("wait", h6)] and (feed.hits, feed.syncs) == (2, 4)
    # the same rows in another order are another batch layout: not a hit
    step(perm[0:4], perm[4:8])
    step(perm[4:8][::-1].copy(), None)
    assert (feed.hits, feed.syncs) == (2, 6)
    # with prefetch off every step stages synchronously and nothing is staged ahead
    off = HostFeed(StubStager(), prefetch=False)
    for i in range(3):
        off.begin(perm[4 * i:4 * i + 4])
        off.end(perm[4 * i + 4:4 * i + 8])
    assert (off.hits, off.syncs) == (0, 3) and [e for e in off.stager.log if e[0] == "stage"] == [
        ("stage", 0, 4), ("stage", 1, 4), ("stage", 0, 4)]


# ------------------------------------------------------------------------------------ index stream and resume
def _host_member(tmp_path, cid=0, seed=1):
    m = _model(tmp_path, cid=cid, seed=seed, use_synthetic_data="learnable", imagenet_data="host")
    ds = m.dataset()
    ds.hip_augment = True  # hand out index batches as on the GPU (they are never materialised here)
    return m, ds


def test_index_stream_announces_and_resumes(tmp_path, fresh_engines):
    m, ds = _host_member(tmp_path)
    n, b = ds.num_train, 4
    assert isinstance(ds, HostImageNetDataset) and n == 256
    batches = [m._batch(ds, None) for _ in range(5)]
    assert all(isinstance(x, IndexBatch) and x.idx.device.type == "cpu" and len(x) == b for x in batches)
    assert m._perm.device.type == "cpu" and m._gen.device.type == "cpu"
    for cur, nxt in zip(batches, batches[1:]):
        assert torch.equal(cur.next_rows, nxt.idx)  # every announcement is the next request
    state = json.loads(json.dumps(m.stream_state()))  # the resume table is JSON
    assert state["data"]["perm_pos"] == 5 * b
    want = [m._batch(ds, None).idx.clone() for _ in range(3)]
    m.release()
    from distributedtf_amd.models.engine_model import EngineModel
    EngineModel._engines.clear()
    r = _model(tmp_path, cid=0, seed=99, use_synthetic_data="learnable", imagenet_data="host")
    assert r.dataset() is ds
    r.restore_stream_state(state)
    got = [r._batch(ds, None).idx.clone() for _ in range(3)]
    assert all(torch.equal(u, v) for u, v in zip(want, got))
    assert json.loads(json.dumps(r.stream_state()))["data"]["perm_pos"] == 8 * b
    # the epoch end announces nothing, and the next epoch is another permutation of every row
    r._perm_pos = n - 2 * b
    last2, last = r._batch(ds, None), r._batch(ds, None)
    assert last2.next_rows is not None and torch.equal(last2.next_rows, last.idx) and last.next_rows is None
    first = r._batch(ds, None)
    assert r._perm_pos == b and sorted(r._perm.tolist()) == list(range(n)) and first.next_rows is not None
    r.release()


# ------------------------------------------------------------------------------------------------- the stager
def test_stager_stages_rows_and_shuts_down():
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, (23, 6, 6, 3), dtype=np.uint8)
    before = {t.ident for t in threading.enumerate()}
    st = RowStager(images, "cpu", threads=3)
    assert st.threads_alive() == 3 and all(t.daemon for t in st._threads)
    with pytest.raises(AssertionError):
        st.stage([0], 0)  # no capacity yet
    st.ensure(20)
    assert st.cap == 20 and st.generation == 1 and st.nbytes == 2 * 20 * 108
    st.dev.fill_(255)
    rows = np.array([22, 0, 5, 5, 1, 9, 3, 17, 4, 4, 21, 2, 8, 6, 7, 10, 11], dtype=np.int64)  # 17: ragged parts
    st.stage(rows, 1)
    st.stage(rows[:1], 0)
    st.wait_copied(1)
    st.wait_copied(0)
    assert np.array_equal(st.dev[1, :17].numpy(), images[rows]) and bool((st.dev[1, 17:] == 255).all())
    assert np.array_equal(st.dev[0, :1].numpy(), images[rows[:1]]) and bool((st.dev[0, 1:] == 255).all())
    with pytest.raises(AssertionError):
        st.stage([23], 0)  # a row outside the set never reaches a gather thread
    st.ensure(10)
    assert st.cap == 20 and st.generation == 1  # never shrinks
    st.ensure(24)
    assert st.cap == 24 and st.generation == 2
    st.close()
    assert st.threads_alive() == 0
    st.close()  # idempotent
    assert {t.ident for t in threading.enumerate()} <= before
    with pytest.raises(RuntimeError, match="closed"):
        st.stage([1], 0)


def test_dropped_dataset_leaves_no_thread(tmp_path):
    import gc
    a = _write(tmp_path, n=9, s=8)
    before = {t.ident for t in threading.enumerate()}
    ds = HostImageNetDataset(a["train_images"], a["train_labels"], a["val_images"], a["val_labels"], "cpu",
                             out_size=8)
    threads = list(ds.feed.stager._threads)
    assert threads and all(t.is_alive() and t.daemon for t in threads)
    ds.feed.begin(np.array([1, 2, 3]))
    ds.feed.end(None)
    del ds
    gc.collect()
    for t in threads:
        t.join(5)
    assert not any(t.is_alive() for t in threads)
    assert {t.ident for t in threading.enumerate()} <= before
