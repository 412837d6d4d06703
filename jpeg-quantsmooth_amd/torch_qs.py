"""do_quantsmooth on PyTorch device tensors: the device-resident job route of include/jpegqs_hip.h
(qs_hip_do_quantsmooth_device) for coefficients that already live on the GPU.

    res = torch_qs.quantsmooth_(coefs, quants, flags, niter, hsamp=[2, 1, 1], vsamp=[2, 1, 1], colorspace=3,
                                image_size=(1920, 1080))
    stop = int(res["stop"])          # the reference's return value (reading it synchronises)

Each coefficient array is a contiguous int16 CUDA tensor of shape (hblk, wblk, 64), rewritten in place.  The job is
enqueued on torch.cuda.current_stream() with no host synchronisation and no allocation outside torch's allocator, so
it can be captured into a torch.cuda.graph: run it once outside the capture (that prepares the workspace), then
capture a call that passes the same `workspace=`.

    res = torch_qs.quantsmooth_batch_([dict(coefs=..., quants=..., hsamp=..., ...), ...], flags, niter)
    stops = res["stop"]              # one int32 per image; res["images"][i] has image i's coef_up, quants, ...

runs many images in one call, their planes sharing kernel launches (qs_hip_do_quantsmooth_device_batch).

torch is imported on first use only: importing the package does not need it."""
from __future__ import annotations

import numpy as np

from .hipqs import HipQS

_HIP = None


def _hip() -> HipQS:
    global _HIP
    if _HIP is None:
        _HIP = HipQS()
    return _HIP


class Workspace:
    """device workspace of one job geometry: a torch uint8 tensor plus what it was prepared for"""

    def __init__(self, buf, key=None):
        self.buf, self.key = buf, key

    @property
    def nbytes(self) -> int:
        return int(self.buf.numel())


def _key(job, flags, niter):
    """what the workspace layout and its constants depend on: everything but the array addresses"""
    from .hipqs import Job
    g = Job.from_buffer_copy(job)
    for ci in range(4):
        g.coef[ci] = None
    g.coef_up[0] = g.coef_up[1] = None
    return (bytes(g), int(flags), int(niter))


def _check_tensors(coefs, torch, who="quantsmooth_"):
    if not isinstance(coefs, (list, tuple)) or not 1 <= len(coefs) <= 4:
        raise ValueError(f"{who}: coefs must be a list of 1..4 tensors")
    dev = None
    for ci, t in enumerate(coefs):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: component {ci} is not a torch.Tensor")
        if t.dtype != torch.int16:
            raise TypeError(f"{who}: component {ci} has dtype {t.dtype}, expected torch.int16")
        if t.dim() != 3 or t.shape[2] != 64 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"{who}: component {ci} has shape {tuple(t.shape)}, expected (hblk, wblk, 64)")
        if not t.is_contiguous():
            raise ValueError(f"{who}: component {ci} is not contiguous")
        if not t.is_cuda:
            raise ValueError(f"{who}: component {ci} is on {t.device}, expected a CUDA (HIP) device tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{who}: component {ci} is on {t.device}, component 0 on {dev}")
    return dev


def _check_quants(quants, n, who="quantsmooth_"):
    if len(quants) != n:
        raise ValueError(f"{who}: one quant table (or None) per component")
    qs = [None if q is None else np.asarray(q, dtype=np.int64).reshape(-1) for q in quants]
    for ci, q in enumerate(qs):
        if q is not None and (q.size != 64 or q.min() < 0 or q.max() > 0xFFFF):
            raise ValueError(f"{who}: quant table {ci} must be 64 values in 0..65535")
    return qs


def _enqueue(jobs, tables, dev, flags, niter, workspace, who, single):
    """what quantsmooth_ (single: the single-job calls) and quantsmooth_batch_ share: the workspace, prepared outside
    any capture when the jobs changed; the replacement chroma tensors; the run on the current stream; what it reports"""
    import torch
    hip = _hip()
    if single:
        arg, prepare, run = jobs[0], hip.device_job_prepare, hip.do_quantsmooth_device
        per = [hip.device_job_info(arg, flags, niter)]
        total = per[0]["workspace_bytes"]
    else:
        arg, prepare, run = jobs, hip.device_batch_prepare, hip.do_quantsmooth_device_batch
        per, total = hip.device_batch_info(jobs, flags, niter)
    key = (single,) + tuple(_key(job, flags, niter) for job in jobs)     # (a job alone is laid out unlike a batch of one)
    stream = torch.cuda.current_stream(dev)
    if workspace is None or workspace.key != key:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: inside a graph capture the workspace must come from an earlier call of the same "
                               f"{'job' if single else 'batch'} (workspace=res['workspace']): preparing one synchronises")
        if workspace is None or workspace.nbytes < total or workspace.buf.device != dev:
            workspace = Workspace(torch.empty(max(1, total), dtype=torch.uint8, device=dev))
        prepare(arg, flags, niter, workspace.buf.data_ptr(), workspace.nbytes, stream.cuda_stream)
        workspace.key = key
    ups = []
    for job, inf in zip(jobs, per):
        up = None
        if inf["up_wblk"] > 0:
            up = [torch.empty((inf["up_hblk"], inf["up_wblk"], 64), dtype=torch.int16, device=dev) for _ in range(2)]
            job.coef_up[0], job.coef_up[1] = up[0].data_ptr(), up[1].data_ptr()
        ups.append(up)
    stop = torch.empty(len(jobs), dtype=torch.int32, device=dev)
    run(arg, flags, niter, workspace.buf.data_ptr(), workspace.nbytes, stop.data_ptr(), stream.cuda_stream)
    out = []
    for job, qs, up in zip(jobs, tables, ups):
        qout = [None if q is None else np.array(job.quant[ci][:], dtype=np.uint16) for ci, q in enumerate(qs)]
        out.append(dict(coef_up=up, quants=qout, hsamp0=int(job.out_hsamp0), vsamp0=int(job.out_vsamp0)))
    return stop, out, workspace


def quantsmooth_(coefs, quants, flags: int, niter: int, *, hsamp=None, vsamp=None, colorspace=None,
                 image_size=None, workspace: Workspace | None = None) -> dict:
    """The reference's do_quantsmooth on `coefs` in place (see the module text).

    quants[ci]: 64 quantisers (natural order) or None (component without a table).  Returns a dict:
      stop       int32 device tensor of one element: the reference's return value (0 done, 1 stopped)
      coef_up    UPSAMPLE_UV: the two replacement chroma tensors (luma geometry), else None
      quants     the output quant tables (all ones where a table was given, as the reference leaves them)
      hsamp0, vsamp0   component 0's output sampling factors
      workspace  the Workspace used; pass it again (also inside a graph capture) for jobs of the same geometry
    coef_up, hsamp0 and vsamp0 describe the result when `stop` reads 0; when it reads 1 the reference drops the
    replacement chroma and component 0 keeps its sampling factors (coef_up's contents are then meaningless)."""
    import torch
    dev = _check_tensors(coefs, torch)
    qs = _check_quants(quants, len(coefs))
    job = _hip().device_job([t.data_ptr() for t in coefs], [tuple(t.shape[:2]) for t in coefs], qs, hsamp=hsamp,
                            vsamp=vsamp, colorspace=colorspace, image_size=image_size)
    stop, (out,), workspace = _enqueue([job], [qs], dev, flags, niter, workspace, "quantsmooth_", True)
    return dict(stop=stop, **out, workspace=workspace)


def quantsmooth_batch_(images, flags: int, niter: int, *, workspace: Workspace | None = None) -> dict:
    """quantsmooth_ on many images in one call (qs_hip_do_quantsmooth_device_batch): their planes share kernel launches,
    so a batch of small or medium images fills the GPU where one image does not.  Results are quantsmooth_'s, image by
    image, bit for bit.

    images[i]: a dict with quantsmooth_'s per-image arguments -- coefs, quants and optionally hsamp, vsamp, colorspace,
    image_size.  One flags / niter setting for the whole batch.  All tensors on one device, none of them twice.
    Returns a dict:
      stop       int32 device tensor of len(images) elements: stop[i] is image i's return value (0 done, 1 stopped)
      images     per image: dict(coef_up, quants, hsamp0, vsamp0), as quantsmooth_ returns them
      workspace  the Workspace used; pass it again (also inside a graph capture) for a batch of the same geometry"""
    import torch
    who = "quantsmooth_batch_"
    if not isinstance(images, (list, tuple)) or not images:
        raise ValueError(f"{who}: images must be a non-empty list of dicts")
    dev, seen, jobs, tables = None, set(), [], []
    hip = _hip()
    for i, im in enumerate(images):
        if not isinstance(im, dict) or "coefs" not in im or "quants" not in im:
            raise ValueError(f"{who}: image {i} must be a dict with coefs and quants")
        coefs = im["coefs"]
        if isinstance(coefs, (list, tuple)) and coefs:      # (the tables first: they need no device)
            qs = _check_quants(im["quants"], len(coefs), who=f"{who}: image {i}")
        d = _check_tensors(coefs, torch, who=f"{who}: image {i}")
        if dev is None:
            dev = d
        elif d != dev:
            raise ValueError(f"{who}: image {i} is on {d}, image 0 on {dev}")
        for t in coefs:
            if t.data_ptr() in seen:
                raise ValueError(f"{who}: image {i} passes a tensor (or its storage) that appears earlier in the batch")
            seen.add(t.data_ptr())
        tables.append(qs)
        jobs.append(hip.device_job([t.data_ptr() for t in coefs], [tuple(t.shape[:2]) for t in coefs], qs,
                                   hsamp=im.get("hsamp"), vsamp=im.get("vsamp"), colorspace=im.get("colorspace"),
                                   image_size=im.get("image_size")))
    stop, out, workspace = _enqueue(jobs, tables, dev, flags, niter, workspace, who, False)
    return dict(stop=stop, images=out, workspace=workspace)
