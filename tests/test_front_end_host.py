"""The steps the torch front end and the ctypes binding share, on the host: torch_qs's workspace step (_prepared) with
CPU tensors and a counted prepare, its block shapes against libjpeg's formulas, and hipqs's table filler, name maps and
pointer arrays through the public calls that use them.  No device is needed."""
import types

import pytest

import jpegqs_pkg

pkg = jpegqs_pkg.load()
torch = pytest.importorskip("torch")
tq, hipqs = pkg.torch_qs, pkg.hipqs
CPU = torch.device("cpu")


# ---- the workspace step ------------------------------------------------------------------------------------------------

class Prepare:
    """a prepare callable that records what it was handed"""

    def __init__(self):
        self.calls = []

    def __call__(self, ptr, nbytes, stream):
        self.calls.append((ptr, nbytes, stream))


@pytest.fixture
def capturing(monkeypatch):
    """torch.cuda as the step sees it: no capture unless state["on"], and a current stream with a handle"""
    state = dict(on=False)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["on"])
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(cuda_stream=77))
    return state


def _step(ws, key, total, prep, in_place=True, same="on the same geometry and tables (workspace=...)"):
    return tq._prepared(ws, key, total, CPU, prep, "stage", same, in_place=in_place)


@pytest.mark.parametrize("in_place", [True, False])
def test_workspace_step_reuses_prepares_and_grows(capturing, in_place):
    prep = Prepare()
    ws = _step(None, ("a", 1), 100, prep, in_place)
    assert isinstance(ws, tq.Workspace) and ws.key == ("a", 1) and ws.nbytes >= 100 and ws.buf.dtype == torch.uint8
    assert prep.calls == [(ws.buf.data_ptr(), ws.nbytes, 77)]
    buf = ws.buf
    # the same key: nothing is prepared, the buffer stays
    assert _step(ws, ("a", 1), 100, prep, in_place) is ws and ws.buf is buf and len(prep.calls) == 1
    # a new key that fits: one prepare into the same buffer of the same object
    assert _step(ws, ("b", 2), 60, prep, in_place) is ws and ws.buf is buf and ws.key == ("b", 2)
    assert prep.calls[1:] == [(buf.data_ptr(), buf.numel(), 77)]
    # a new key that does not fit: a new buffer -- in the same object, or (the smoothing calls) in a new one
    size = ws.nbytes
    got = _step(ws, ("c", 3), size + 1, prep, in_place)
    assert got.key == ("c", 3) and got.nbytes >= size + 1 and got.buf is not buf and len(prep.calls) == 3
    assert prep.calls[2] == (got.buf.data_ptr(), got.nbytes, 77)
    if in_place:
        assert got is ws
    else:
        assert got is not ws and ws.buf is buf and ws.nbytes == size and ws.key == ("b", 2)


def test_an_empty_workspace_is_filled_in_place(capturing):
    prep, ws = Prepare(), tq.Workspace()
    assert _step(ws, ("a",), 10, prep) is ws and ws.nbytes >= 10 and ws.key == ("a",) and len(prep.calls) == 1


@pytest.mark.parametrize("in_place", [True, False])
def test_no_bytes_still_give_a_buffer_of_one(capturing, in_place):
    prep = Prepare()
    ws = _step(None, ("a",), 0, prep, in_place)
    assert ws.nbytes == 1 and prep.calls == [(ws.buf.data_ptr(), 1, 77)]
    if in_place:
        ws = _step(tq.Workspace(), ("a",), 0, prep)
        assert ws.nbytes == 1


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("same", ["on the same geometry and tables (workspace=...)",
                                  "on the same geometry, scans and tables (workspace=...)",
                                  "with the same geometry, scripts and markers (workspace=...)",
                                  "of the same batch (workspace=res['workspace'])"])
def test_a_capture_refuses_to_prepare(capturing, in_place, same):
    prep = Prepare()
    ws = _step(None, ("a",), 10, prep, in_place)
    capturing["on"] = True
    assert _step(ws, ("a",), 10, prep, in_place, same) is ws          # the prepared key passes
    buf = ws.buf
    for passed in (ws, None):
        with pytest.raises(RuntimeError) as e:
            _step(passed, ("b",), 10, prep, in_place, same)
        assert str(e.value) == (f"stage: inside a graph capture the workspace must come from an earlier call {same}: "
                                f"preparing one synchronises")
    assert len(prep.calls) == 1 and ws.key == ("a",) and ws.buf is buf


# ---- block shapes --------------------------------------------------------------------------------------------------------

def _libjpeg_shapes(w, h, hsamp, vsamp):
    """jpeg_read_coefficients' height_in_blocks x width_in_blocks, as the readers spelled them"""
    mh, mv = max(hsamp), max(vsamp)
    return [(-(-h * vsamp[ci] // (8 * mv)), -(-w * hsamp[ci] // (8 * mh))) for ci in range(len(hsamp))]


@pytest.mark.parametrize("w,h,hsamp,vsamp,want", [
    (17, 9, [2, 1, 1], [2, 1, 1], [(2, 3), (1, 2), (1, 2)]),
    (8, 8, [1], [1], [(1, 1)]),
    (33, 1, [4, 1, 1], [1, 1, 1], [(1, 5), (1, 2), (1, 2)]),
    (33, 18, [2, 1, 1], [1, 1, 1], [(3, 5), (3, 3), (3, 3)]),
    (33, 18, [1, 1, 1], [2, 1, 1], [(3, 5), (2, 5), (2, 5)]),
    (1, 1, [2], [2], [(1, 1)]),
])
def test_block_shapes(w, h, hsamp, vsamp, want):
    assert tq._block_shapes(w, h, hsamp, vsamp) == want == _libjpeg_shapes(w, h, hsamp, vsamp)


def test_mcu_geometry_counts_the_blocks_of_a_1x1_component():
    for w, h in ((17, 9), (33, 1), (640, 481)):
        for hs, vs in (([2, 1, 1], [2, 1, 1]), ([4, 1, 1], [1, 1, 1]), ([1, 1, 1], [2, 1, 1])):
            hb, wb = tq._block_shapes(w, h, hs, vs)[1]
            assert tq._mcu_geometry(hs, vs, (w, h)) == (wb, wb * hb)
        assert tq._mcu_geometry([2], [2], (w, h)) == (-(-w // 8), -(-w // 8) * -(-h // 8))    # one block per MCU


# ---- the single-image wrappers' helpers -------------------------------------------------------------------------------------

def test_single_image_helpers():
    assert tq._batch_result(None) is None and tq._outs_of(None) is None
    res = dict(stop="s", quants=[1])
    assert tq._batch_result(res) == dict(stop="s", images=[res]) and tq._outs_of(res) == [res]


# ---- hipqs -----------------------------------------------------------------------------------------------------------------

TABLE = ([0, 0, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [3, 250, 7])


def _scan(dc=None, ac=None):
    return dict(comps=[0], ss=0, se=0, ah=0, al=0, dc_tbl=[0], ac_tbl=[0], dc=dc, ac=ac, restart_interval=0, offset=0)


def test_the_three_table_records_are_filled_alike():
    first = hipqs.HipQS.huff_tables(dc={1: TABLE}, ac={0: TABLE})
    ro = hipqs.HipQS.read_opts(dc={1: TABLE}, ac={0: TABLE})
    rp = hipqs.HipQS.read_prog_opts([_scan(dc={1: TABLE}, ac={0: TABLE})])._scans[0]
    want_bits, want_vals = bytes(TABLE[0]), bytes(TABLE[1]) + bytes(253)
    for rec, ids in ((first, 2), (ro, 4), (rp, 4)):
        for arr, has, k in ((rec.dc, rec.has_dc, 1), (rec.ac, rec.has_ac, 0)):
            assert bytes(arr[k].bits) == want_bits and bytes(arr[k].huffval) == want_vals
            assert list(has) == [1 if t == k else 0 for t in range(ids)]
            assert bytes(arr[1 - k]) == bytes(273)                    # the table left out stays empty
    assert bytes(first.dc[1]) == bytes(ro.dc[1]) == bytes(rp.dc[1]) and bytes(first.ac[0]) == bytes(ro.ac[0]) == bytes(rp.ac[0])


@pytest.mark.parametrize("name,make,bad_id,span", [
    ("huff_tables", lambda t: hipqs.HipQS.huff_tables(ac=t), 2, "0 or 1"),
    ("read_opts", lambda t: hipqs.HipQS.read_opts(ac=t), 4, "0..3"),
    ("read_prog_opts", lambda t: hipqs.HipQS.read_prog_opts([_scan(ac=t)]), 4, "0..3"),
])
def test_each_table_record_refuses_in_its_own_name(name, make, bad_id, span):
    for tabs in ({bad_id: TABLE}, {0: (TABLE[0][:16], TABLE[1])}, {0: (TABLE[0], [0] * 257)}):
        with pytest.raises(ValueError) as e:
            make(tabs)
        assert str(e.value) == f"{name}: table {span}, bits[17], at most 256 symbols"
    make({bad_id - 1: (TABLE[0], [0] * 256)})                         # the last id and 256 symbols pass


def _jobs(n=2):
    return [hipqs.HipQS.device_job([1], [(2, 2)], [[1] * 64], image_size=(16, 16)) for _ in range(n)]


def test_name_maps_refuse_with_their_own_words(hip):
    for info, what, field, names in ((hip.decode_batch_info, "decode", "upsampling", ["dct", "triangle"]),
                                     (hip.compress_batch_info, "compress", "downsampling", ["box", "dct"])):
        with pytest.raises(ValueError) as e:
            info(_jobs(), opts=[names[1]])
        assert str(e.value) == f"{what} opts: 1 entries for 2 jobs"
        with pytest.raises(ValueError) as e:
            info(_jobs(), opts=[None, "nonsense"])
        assert str(e.value) == f"{what} opts: {field} 'nonsense' (one of {names})"
        plain = info(_jobs())
        assert info(_jobs(), opts=[None, names[0]]) == plain == info(_jobs(), opts=[0, names[0]])
    arr, keep = hipqs._named_ptrs(*hipqs._DECODE_MODES, [None, "triangle", hipqs.DecodeOpts(1)], 3)
    assert not arr[0] and arr[1].contents.upsampling == arr[2].contents.upsampling == hipqs.UPSAMPLE_TRIANGLE
    assert keep[0] is None and isinstance(keep[1], hipqs.DecodeOpts)


def test_pointer_arrays_have_a_slot_at_least(hip):
    assert len(hip._job_ptrs([])) == 1 and not hip._job_ptrs([])[0]
    jobs = _jobs(3)
    arr = hip._job_ptrs(jobs[:2] + [None])
    assert len(arr) == 3 and arr[0].contents.image_width == 16 and not arr[2]
    assert hip._opt_ptrs(None, 3) == (None, None)
    with pytest.raises(ValueError, match="one options entry"):
        hip._opt_ptrs([(1, 0)], 2)
    with pytest.raises(ValueError, match="one ReadOpts per job"):
        hip.read_batch_info(jobs, [hipqs.HipQS.read_opts()])


def test_encode_prepare_takes_one_table_record_or_none_per_job(hip):
    """(a list shorter than the jobs used to be padded with NULL; it is refused before the library is called)"""
    for tables in ([None], [None, None, None]):
        with pytest.raises(ValueError) as e:
            hip.encode_batch_prepare(_jobs(2), tables, 0, 0)
        assert str(e.value) == "one HuffTables (or None) per job"
