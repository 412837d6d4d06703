"""What the entropy coder's info calls answer, number by number: qs_hip_encode_device_batch_info[_opts],
qs_hip_encode_files_scratch_bytes and qs_hip_encode_progressive_device_batch_info over a small grid of batches, restart
options and scan scripts, against tests/golden/encode_plan_record.json -- the answers of the library before its two host
drivers (csrc/qs_encode_job.cpp, csrc/qs_encode_prog_job.cpp) took their restart rule, workspace layout and scratch
layout from one header (csrc/qs_encode_plan.h).  Workspace sizes are the sum of every array the layout takes, so a
changed array, order or capacity shows here; so do the code and the text of every refusal.  No call asks for a device.

QS_RECORD_ENCODE_PLAN=1 rewrites the record from the library in the tree: only for a change that is meant to move it."""
import json
import os
from pathlib import Path

RECORD = Path(__file__).resolve().parent / "golden" / "encode_plan_record.json"
Q = [16] * 64
BASE = (0x100000, 0x200000, 0x300000, 0x400000)


def _batches(hip):
    """{name: (jobs, the MCUs of the scan that carries all components at the original sampling)}"""

    def job(shapes, hs, vs, cs, size):
        n = len(shapes)
        return hip.device_job(list(BASE[:n]), list(shapes), [Q] * n, hsamp=list(hs), vsamp=list(vs), colorspace=cs,
                              image_size=size)

    def ycc(up=False):
        j = job([(4, 4), (2, 2), (2, 2)], (2, 1, 1), (2, 1, 1), 3, (32, 32))
        if up:                                              # replacement chroma of 4 x 4 blocks: two variants
            j.up_wblk = j.up_hblk = 4
            j.coef_up[0], j.coef_up[1] = 0x900000, 0xa00000
        return j

    return {
        "gray_8x8": ([job([(1, 1)], [1], [1], 1, (8, 8))], 1),                     # one block
        "gray_2056x8": ([job([(1, 257)], [1], [1], 1, (2056, 8))], 257),           # the second workgroup
        "ycc420_32x32": ([ycc()], 4),
        "ycc420_32x32_replacement_chroma": ([ycc(up=True)], 4),
        # 4x2 + 1x1 + 1x1 + 1x1: 11 blocks in an MCU (tests/test_stage_errors.py)
        "cmyk_11_blocks": ([job([(2, 4), (1, 1), (1, 1), (1, 1)], [4, 1, 1, 1], [2, 1, 1, 1], 4, (32, 16))], 1),
        "gray_65500x80": ([job([(10, 8188)], [1], [1], 1, (65500, 80))], 81880),   # 9 rows of MCUs pass 65535
        "ycc420_32x32_x33": ([ycc() for _ in range(33)], 4),                       # the second launch chunk
    }


def _answer(pkg, call):
    """ok: [[a job's answer, how many jobs in a row gave it], ...] and the sizes of the batch"""
    try:
        per, *sizes = call()
    except pkg.hipqs.QsHipError as e:
        return dict(error=[e.code, str(e)])
    runs = []
    for p in per:
        if runs and runs[-1][0] == p:
            runs[-1][1] += 1
        else:
            runs.append([p, 1])
    return dict(ok=[runs] + sizes)


def _record(pkg, hip):
    jf = pkg.jpeg_file
    out = {"scratch_bytes": {str(n): hip.encode_files_scratch_bytes(n) for n in (-1, 0, 1, 2, 33, 257)}}
    for name, (jobs, mcus) in _batches(hip).items():
        n, ncomp, cs = len(jobs), jobs[0].ncomp, jobs[0].colorspace
        scripts = {"spectral": (jf.spectral_script(ncomp), False),
                   "simple": (jf.simple_progression(ncomp, cs), False),
                   "simple_refinement": (jf.simple_progression(ncomp, cs), True),
                   "dc_only": ([jf.scan(range(ncomp), 0, 0)], False),
                   "dc_of_each_component": ([jf.scan([c], 0, 0) for c in range(ncomp)], False)}
        out[f"{name}|info"] = _answer(pkg, lambda: hip.encode_batch_info(jobs))
        restarts = {"none": None, "interval_1": (1, 0), "interval_mcus": (mcus, 0), "rows_1": (0, 1), "rows_9": (0, 9),
                    "interval_65536": (65536, 0), "rows_-1": (0, -1)}
        for rname, rst in restarts.items():
            out[f"{name}|{rname}|info_opts"] = _answer(pkg, lambda: hip.encode_batch_info(jobs, opts=[rst] * n))
            for sname, (script, refinement) in scripts.items():
                popts = [hip.prog_opts(script, *(rst or (0, 0)), refinement=refinement) for _ in range(n)]
                out[f"{name}|{rname}|progressive|{sname}"] = _answer(pkg, lambda: hip.encode_progressive_info(jobs, popts))
    return json.loads(json.dumps(out))                      # (tuples as lists, as the record reads back)


def test_info_calls_answer_what_the_record_holds(pkg, hip):
    got = _record(pkg, hip)
    if os.environ.get("QS_RECORD_ENCODE_PLAN") == "1":
        RECORD.write_text(json.dumps(got, indent=0, sort_keys=True) + "\n")
    want = json.loads(RECORD.read_text())
    assert sorted(got) == sorted(want)
    wrong = [f"{k}:\n    want {want[k]}\n    got  {got[k]}" for k in want if got[k] != want[k]]
    assert not wrong, f"{len(wrong)} of {len(want)} answers:\n" + "\n".join(wrong[:20])
    # the grid holds what it is meant to hold: accepted and refused answers of every call
    assert want["cmyk_11_blocks|info"]["error"][0] == -4
    assert "ok" in want["cmyk_11_blocks|none|progressive|dc_of_each_component"]
    assert want["gray_65500x80|rows_9|progressive|spectral"]["ok"][0][0][0]["interval"][0] == 65535
    assert want["ycc420_32x32_x33|none|info_opts"]["ok"][0][0][1] == 33
    assert "error" in want["ycc420_32x32|interval_65536|info_opts"] and "error" in want["ycc420_32x32|rows_-1|info_opts"]
