"""CPU tests of the device-resident batch route (include/jpegqs_hip.h: qs_hip_device_batch_info,
qs_hip_device_batch_prepare, qs_hip_do_quantsmooth_device_batch) and its torch front end
(torch_qs.quantsmooth_batch_): the per-job plan against the single-job call, the workspace size and argument checking."""
import numpy as np
import pytest

from helpers import golden_names, load_golden

EINVAL, ENODEV = -2, -1
FAKE_WS, FAKE_STOP = 0x40000000, 0x8000


def _job(hip, j, base, coef_up=None):
    """a qs_hip_job over (fake, disjoint) device addresses with the golden's geometry: these calls never touch them"""
    shapes = [c.shape[:2] for c in j["coefs"]]
    return hip.device_job([base + 0x1000000 * ci for ci in range(len(shapes))], shapes, j["quants"], coef_up=coef_up,
                          **j["kw"])


def _batch(hip, names, with_up=True):
    """one job per golden, each at its own fake addresses (replacement chroma arrays where the job needs them)"""
    jobs = []
    for i, name in enumerate(names):
        j, _ = load_golden(name)
        base = 0x100000000 * (i + 1)
        job = _job(hip, j, base)
        if with_up and hip.device_job_info(job, j["flags"], j["niter"])["up_wblk"] > 0:
            job = _job(hip, j, base, coef_up=(base + 0x10000000, base + 0x20000000))
        jobs.append(job)
    return jobs


def _by_setting():
    """the goldens grouped by (flags, niter): the batches a caller could form"""
    groups = {}
    for name in golden_names():
        j, _ = load_golden(name)
        groups.setdefault((j["flags"], j["niter"]), []).append(name)
    return groups


def test_abi_lists_the_batch_calls(pkg):
    from jpeg_quantsmooth_amd import hipqs
    for name in ("qs_hip_device_batch_info", "qs_hip_device_batch_prepare", "qs_hip_do_quantsmooth_device_batch"):
        assert name in hipqs.ABI


@pytest.mark.parametrize("setting", sorted(_by_setting()))
def test_batch_info_equals_the_single_job_info(hip, setting):
    """per_job[i] is what qs_hip_device_job_info reports for job i; the batch needs at least the jobs' workspaces"""
    flags, niter = setting
    names = _by_setting()[setting]
    jobs = _batch(hip, names)
    per, total = hip.device_batch_info(jobs, flags, niter)
    singles = [hip.device_job_info(job, flags, niter) for job in jobs]
    assert per == singles
    assert total >= sum(s["workspace_bytes"] for s in singles) + 4 * len(jobs)


def test_mixed_batch_of_every_golden(hip):
    """every golden in one batch under each golden's setting: the plan of each job does not depend on the others"""
    names = golden_names()
    for flags, niter in sorted(_by_setting()):
        jobs = _batch(hip, names)
        per, total = hip.device_batch_info(jobs, flags, niter)
        singles = [hip.device_job_info(job, flags, niter) for job in jobs]
        assert per == singles, (flags, niter)
        assert total >= sum(s["workspace_bytes"] for s in singles)


def _six(hip):
    """six q6 jobs: 4:2:0 goldens (replacement chroma) and a grey one"""
    names = [n for n in golden_names() if "q6" in n][:5] + [n for n in golden_names() if n.startswith("gray")][:1]
    assert len(names) == 6, names
    j, _ = load_golden(names[0])
    return _batch(hip, names), j["flags"], j["niter"]


def _code(pkg, fn, *args):
    with pytest.raises(pkg.QsHipError) as ei:
        fn(*args)
    return ei.value.code, str(ei.value)


def test_run_rejects_bad_arguments(hip, pkg):
    """EINVAL, checked before anything is enqueued: no jobs, a null job, a bad geometry in job 3 (named), a short
    workspace, a null stop array, overlapping arrays of two jobs, a missing replacement chroma array"""
    jobs, flags, niter = _six(hip)
    _, total = hip.device_batch_info(jobs, flags, niter)
    run = hip.do_quantsmooth_device_batch
    assert _code(pkg, run, [], flags, niter, FAKE_WS, total, FAKE_STOP)[0] == EINVAL
    code, msg = _code(pkg, run, jobs[:2] + [None] + jobs[3:], flags, niter, FAKE_WS, total, FAKE_STOP)
    assert code == EINVAL and "job 2" in msg
    bad = _six(hip)[0]
    bad[3].wblk[0] = 0
    code, msg = _code(pkg, run, bad, flags, niter, FAKE_WS, total, FAKE_STOP)
    assert code == EINVAL and "job 3" in msg, msg
    code, msg = _code(pkg, hip.device_batch_info, bad, flags, niter)
    assert code == EINVAL and "job 3" in msg, msg
    assert _code(pkg, run, jobs, flags, niter, FAKE_WS, total - 1, FAKE_STOP)[0] == EINVAL
    assert _code(pkg, run, jobs, flags, niter, FAKE_WS + 16, total, FAKE_STOP)[0] == EINVAL
    assert _code(pkg, run, jobs, flags, niter, FAKE_WS, total, 0)[0] == EINVAL
    over = _six(hip)[0]
    over[4].coef[2] = over[1].coef[0] + 128                  # job 4's third array starts inside job 1's luma
    code, msg = _code(pkg, run, over, flags, niter, FAKE_WS, total, FAKE_STOP)
    assert code == EINVAL and "overlap" in msg and "1" in msg and "4" in msg, msg
    same = _six(hip)[0]
    same[5] = same[0]                                        # one job twice
    assert _code(pkg, run, same, flags, niter, FAKE_WS, total, FAKE_STOP)[0] == EINVAL
    noup = _six(hip)[0]
    noup[2].coef_up[1] = None
    code, msg = _code(pkg, run, noup, flags, niter, FAKE_WS, total, FAKE_STOP)
    assert code == EINVAL and "job 2" in msg and "coef_up" in msg, msg
    assert _code(pkg, hip.device_batch_prepare, jobs, flags, niter, FAKE_WS, total - 1)[0] == EINVAL
    assert _code(pkg, hip.device_batch_info, [], flags, niter)[0] == EINVAL


def test_run_without_device_is_enodev(hip, pkg):
    """valid arguments and no device: ENODEV, nothing computed on the CPU"""
    if hip.device_count() > 0:
        pytest.skip("a GPU is present: the fake device addresses of this test must not reach it")
    jobs, flags, niter = _six(hip)
    _, total = hip.device_batch_info(jobs, flags, niter)
    assert _code(pkg, hip.do_quantsmooth_device_batch, jobs, flags, niter, FAKE_WS, total, FAKE_STOP)[0] == ENODEV
    assert _code(pkg, hip.device_batch_prepare, jobs, flags, niter, FAKE_WS, total)[0] == ENODEV


def test_torch_front_end_checks_arguments(pkg):
    """an empty batch, a non-dict entry, host tensors, a wrong dtype and a wrong number of tables are refused before the
    library is called (image index in the message)"""
    import torch
    from jpeg_quantsmooth_amd import torch_qs
    q = np.full(64, 16, dtype=np.uint16)
    dev = dict(coefs=[torch.zeros((4, 4, 64), dtype=torch.int16)], quants=[q])
    with pytest.raises(ValueError, match="non-empty"):
        torch_qs.quantsmooth_batch_([], 0, 3)
    with pytest.raises(ValueError, match="image 0 must be a dict"):
        torch_qs.quantsmooth_batch_([[dev["coefs"][0]]], 0, 3)
    with pytest.raises(ValueError, match="image 0: component 0 .*CUDA"):
        torch_qs.quantsmooth_batch_([dev], 0, 3)
    with pytest.raises(TypeError, match="image 0: component 0 .*int16"):
        torch_qs.quantsmooth_batch_([dict(dev, coefs=[torch.zeros((4, 4, 64), dtype=torch.int32)])], 0, 3)
    with pytest.raises(ValueError, match="image 0: one quant table"):
        torch_qs.quantsmooth_batch_([dict(dev, quants=[q, q])], 0, 3)
    with pytest.raises(ValueError, match="image 0: coefs"):
        torch_qs.quantsmooth_batch_([dict(dev, coefs=[])], 0, 3)
    assert pkg.quantsmooth_batch_ is torch_qs.quantsmooth_batch_
