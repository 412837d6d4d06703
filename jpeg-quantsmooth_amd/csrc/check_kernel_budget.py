#!/usr/bin/env python3
"""Build guard for qs_kernels.hip (csrc/build_stripped.sh): the four recovery kernels -- qs_smooth_plane_kernel and
qs_smooth_set_kernel, each with and without DIAGONALS -- must keep three waves per SIMD and three workgroups per CU with
nothing in scratch.  The luma instantiations hold 144 pixel differences in registers and sit a few registers under the
limit: a toolchain or a source change that tips them over would still build, and run 10-40 % slower on spills or at
two waves per SIMD (LABNOTES.md 4.2).

Reads the code-object metadata the compiler prints into the device assembly (the `amdhsa.kernels` list between
.amdgpu_metadata and .end_amdgpu_metadata) and nothing else -- no instruction is looked at:
    .private_segment_fixed_size == 0      no spills, no scratch
    .vgpr_count <= 168                    512 / 3 registers per lane, in the allocation granule of 8
    .group_segment_fixed_size <= 54613    160 KiB of LDS / 3 workgroups

usage: check_kernel_budget.py <device.s>      exit status 1 (with the offending kernels named) when a budget is missed
"""
import re
import sys

KERNELS = ("qs_smooth_plane_kernel", "qs_smooth_set_kernel")
MAX_VGPRS = 168
MAX_LDS = 160 * 1024 // 3
FIELDS = ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count")


def kernel_records(text):
    """{symbol: {field: int}} of the metadata block"""
    m = re.search(r"^\s*\.amdgpu_metadata\s*$(.*?)^\s*\.end_amdgpu_metadata\s*$", text, re.S | re.M)
    if not m:
        return {}
    # The list is YAML as LLVM prints it: a kernel record opens with "  - .<field>:" (its argument list, whose items sit
    # deeper) and its scalar fields follow at four columns.
    recs, cur = [], None
    for line in m.group(1).split("\n"):
        if re.match(r"  - \.", line):
            cur = {}
            recs.append(cur)
            line = "    " + line[4:]
        f = re.match(r"    \.(\w+):\s*(\S+)\s*$", line)
        if f and cur is not None:
            cur[f.group(1)] = f.group(2)
    return {r["name"]: {k: int(r[k]) for k in FIELDS if k in r} for r in recs if "name" in r}


def main(path):
    recs = {n: r for n, r in kernel_records(open(path).read()).items() if any(k in n for k in KERNELS)}
    if len(recs) != 4 or any(len(r) != len(FIELDS) for r in recs.values()):
        print(f"check_kernel_budget: ERROR: expected the metadata of 4 recovery kernels in {path}, found {sorted(recs)}", file=sys.stderr)
        return 1
    bad = 0
    for n, r in sorted(recs.items()):
        why = []
        if r["private_segment_fixed_size"] != 0:
            why.append(f"{r['private_segment_fixed_size']} B of scratch per lane (spills)")
        if r["vgpr_count"] > MAX_VGPRS:
            why.append(f"{r['vgpr_count']} VGPRs > {MAX_VGPRS} (three waves per SIMD)")
        if r["group_segment_fixed_size"] > MAX_LDS:
            why.append(f"{r['group_segment_fixed_size']} B of LDS > {MAX_LDS} (three workgroups per CU)")
        print(f"check_kernel_budget: {n}: {r['vgpr_count']} VGPRs, {r['private_segment_fixed_size']} B scratch, "
              f"{r['group_segment_fixed_size']} B LDS" + (" -- ERROR: " + "; ".join(why) if why else ""),
              file=sys.stderr if why else sys.stdout)
        bad += bool(why)
    return 1 if bad else 0


# the kernels of the scan reader's split route (qs_kernels_read_split.hip): nothing in scratch -- a lane's bit reader,
# its state and the block it writes to live in registers, the code tables in LDS
SPLIT_READ_KERNELS = ("qrs_map", "qrs_decode", "qrs_count", "qrs_tile_scan", "qrs_write", "qrs_dc_tiles", "qrs_dc_write")
# the decode to pixels (qs_kernels_decode.hip): a lane's block, its IDCT workspace and the rows of the triangle filter
# are arrays indexed by unrolled loops -- they stay in registers only as long as every index is a constant
DECODE_KERNELS = ("qs_decode_kernel", "qs_decode_scaled_kernel")     # (the second: the reduced sizes' kernel)
# the progressive run (qs_kernels_encode_prog.inc): a lane's block is an array indexed by an unrolled walk over the band,
# whose bounds are run-time values -- it stays in registers only as long as every index is a constant
PROG_KERNELS = ("qp_begin", "qp_nofile", "qp_flags", "qp_headscan", "qp_runs", "qp_size", "qp_emit", "qp_frame",
                "qr_flags", "qr_wsum", "qr_wscan", "qr_next", "qr_hop")      # qr_: the refinement scans' own
# the scan reader's progressive route (qs_kernels_read_prog.hip): as for the split route; the job's arrays are reached
# through the kernel arguments, not through a local copy a lane would index
READ_PROG_KERNELS = ("qrp_init", "qrp_check", "qrp_decode")
INSTANCES = {"qp_size": 4, "qp_emit": 2}     # template instantiations of one name (every other kernel: one)


def main_no_scratch(prefix, path):
    """--no-scratch <prefix> <device.s>: every kernel of SPLIT_READ_KERNELS, DECODE_KERNELS, PROG_KERNELS and
    READ_PROG_KERNELS that starts with the prefix is there (in all its instantiations) and has no scratch"""
    want = [k for k in SPLIT_READ_KERNELS + DECODE_KERNELS + PROG_KERNELS + READ_PROG_KERNELS if k.startswith(prefix)]
    recs = kernel_records(open(path).read())
    bad = 0
    for k in want:
        hits = {n: r for n, r in recs.items() if re.search(rf"\d+{k}[EI\d]", n)}
        if len(hits) != INSTANCES.get(k, 1) or any("private_segment_fixed_size" not in r for r in hits.values()):
            count = {1: "one kernel"}.get(INSTANCES.get(k, 1), f"{INSTANCES.get(k, 1)} kernels")
            print(f"check_kernel_budget: ERROR: expected the metadata of {count} {k} in {path}, found {sorted(hits)}", file=sys.stderr)
            bad += 1
            continue
        for n, r in sorted(hits.items()):
            scratch = r["private_segment_fixed_size"]
            print(f"check_kernel_budget: {n}: {r.get('vgpr_count')} VGPRs, {scratch} B scratch, {r.get('group_segment_fixed_size')} B LDS"
                  + (" -- ERROR: scratch" if scratch else ""), file=sys.stderr if scratch else sys.stdout)
            bad += bool(scratch)
    return 1 if bad or not want else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--no-scratch":
        sys.exit(main_no_scratch(sys.argv[2], sys.argv[3]))
    sys.exit(main(sys.argv[1]))
