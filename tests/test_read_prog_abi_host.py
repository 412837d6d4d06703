"""qs_hip_read_prog_device_batch_info on a machine without a GPU: what the progressive route of the scan reader reports
and what it refuses before anything is enqueued."""
import pytest

import jpegqs_pkg

pkg = jpegqs_pkg.load()
from jpeg_quantsmooth_amd import jpeg_file  # noqa: E402

EINVAL, ENOTSUP = -2, -4


@pytest.fixture(scope="module")
def hip():
    return pkg.HipQS()


def scans_of(hip, script, ri=0, tbl=None):
    """the scan records a file of this script would parse to (standard tables in effect, offsets 100 bytes apart)"""
    dc = {t: hip.huff_standard(0, t) for t in (0, 1)}
    ac = {t: hip.huff_standard(1, t) for t in (0, 1)}
    out = []
    for i, (comps, ss, se, ah, al) in enumerate(script):
        t = [(tbl or [0, 1, 1, 0])[c] for c in comps]
        out.append(dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, dc_tbl=t if ss == 0 and not ah else [0] * len(t),
                        ac_tbl=t if ss else [0] * len(t), dc=dc, ac=ac, restart_interval=ri, offset=100 * (i + 1)))
    return out


def job(hip, shapes, hs, vs, size):
    return hip.device_job([0x1000 * (i + 1) for i in range(len(shapes))], shapes, [None] * len(shapes), hsamp=hs, vsamp=vs,
                          colorspace=3 if len(shapes) == 3 else 1, image_size=size)


def refused(hip, j, scans):
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_prog_batch_info([j], [hip.read_prog_opts(scans)])
    return e.value.code, str(e.value)


def test_info_reports_levels_and_per_scan_intervals(hip):
    ycc = job(hip, [(12, 18), (6, 9), (6, 9)], [2, 1, 1], [2, 1, 1], (141, 93))
    script = jpeg_file.simple_progression(3, 3)
    per, nbytes = hip.read_prog_batch_info([ycc, ycc], [hip.read_prog_opts(scans_of(hip, script, ri=7))] * 2)
    assert per[0] == per[1] and nbytes > 0
    assert per[0]["nscans"] == 10 and per[0]["levels"] == 3
    # an interleaved scan counts the frame's 9 x 6 MCUs, a one-component scan its own blocks: 18 x 12 luma, 9 x 6 chroma
    assert per[0]["mcus"] == [54, 216, 54, 54, 216, 216, 54, 54, 54, 216]
    assert per[0]["intervals"] == [8, 31, 8, 8, 31, 31, 8, 8, 8, 31]
    spectral = hip.read_prog_batch_info([ycc], [hip.read_prog_opts(scans_of(hip, jpeg_file.spectral_script(3)))])[0][0]
    assert spectral["levels"] == 1 and spectral["intervals"] == [1] * 7
    gray = job(hip, [(3, 5)], [1], [1], (33, 18))
    twice = [((0,), 0, 0, 0, 2), ((0,), 0, 0, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 0)]
    assert hip.read_prog_batch_info([gray], [hip.read_prog_opts(scans_of(hip, twice))])[0][0]["levels"] == 3


def test_info_refuses_what_the_route_does_not_cover(hip):
    gray_script = [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)]
    # 2056 x 1024 gray without DRI: 257 x 128 = 32 896 blocks in the one interval of every scan
    big = job(hip, [(128, 257)], [1], [1], (2056, 1024))
    code, msg = refused(hip, big, scans_of(hip, gray_script))
    assert code == ENOTSUP and "32896 blocks" in msg and "scan 0" in msg
    per, _ = hip.read_prog_batch_info([big], [hip.read_prog_opts(scans_of(hip, gray_script, ri=257))])
    assert per[0]["intervals"] == [128] * 3
    # exactly the cap is read: 2048 x 1024
    cap = job(hip, [(128, 256)], [1], [1], (2048, 1024))
    assert hip.read_prog_batch_info([cap], [hip.read_prog_opts(scans_of(hip, gray_script))])[0][0]["intervals"] == [1] * 3
    gray = job(hip, [(3, 5)], [1], [1], (33, 18))
    code, msg = refused(hip, gray, scans_of(hip, [((0,), 0, 0, 0, 0)] + [((0,), 1 + i % 63, 1 + i % 63, 0, 0) for i in range(256)]))
    assert code == ENOTSUP and "257 scans" in msg
    code, msg = refused(hip, gray, scans_of(hip, [((0,), 1, 63, 0, 0), ((0,), 0, 0, 0, 0)]))
    assert code == EINVAL and "scan 0" in msg and "DC scan" in msg
    code, msg = refused(hip, gray, scans_of(hip, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 2, 1)]))
    assert code == EINVAL and "scan 2" in msg
    code, msg = refused(hip, gray, scans_of(hip, [((0,), 0, 63, 0, 0)]))
    assert code == ENOTSUP and "progressive" in msg                     # a sequential script
    # a scan that uses a table its record does not hold; a DC refinement names none and needs none
    s = scans_of(hip, gray_script)
    s[1] = dict(s[1], ac={})
    code, msg = refused(hip, gray, s)
    assert code == EINVAL and "scan 1" in msg and "AC table 0" in msg
    s = scans_of(hip, [((0,), 0, 0, 0, 1), ((0,), 0, 0, 1, 0)])
    s[1] = dict(s[1], dc={}, ac={})
    assert hip.read_prog_batch_info([gray], [hip.read_prog_opts(s)])[0][0]["levels"] == 2
    # 14 blocks in the MCU of an interleaved scan; the same frame scan by scan is read
    wide = job(hip, [(8, 8), (8, 8), (8, 8)], [4, 2, 2], [2, 2, 1], (64, 64))
    code, msg = refused(hip, wide, scans_of(hip, [((0, 1, 2), 0, 0, 0, 0)]))
    assert code == ENOTSUP and "14 blocks in an MCU" in msg
    per, _ = hip.read_prog_batch_info([wide], [hip.read_prog_opts(scans_of(hip, [((c,), 0, 0, 0, 0) for c in range(3)]))])
    assert per[0]["levels"] == 1
    # an array narrower than libjpeg's width_in_blocks
    code, _ = refused(hip, job(hip, [(3, 4)], [1], [1], (33, 18)), scans_of(hip, gray_script))
    assert code == EINVAL


def test_run_on_a_workspace_never_prepared_is_refused(hip):
    gray = job(hip, [(3, 5)], [1], [1], (33, 18))
    with pytest.raises(pkg.hipqs.QsHipError) as e:
        hip.read_prog_batch([gray], [0x10000], [100], 0x20000, 0x40000, 1 << 20)
    assert e.value.code == EINVAL and "never prepared" in str(e.value)
