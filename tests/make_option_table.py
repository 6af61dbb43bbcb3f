"""Generates tests/golden/option_table.json: what mpcg_set_option / mpcg_get_option (mpcg_pcg.hip) do with every key.
Run on the GPU box: `python tests/make_option_table.py [--out PATH] [--force]` (an existing table is kept unless --force is given).
tests/test_gpu_options.py records the same table again and compares exactly.  No solve kernel is launched.

Per horizon in KNOTS (state_size 14, max_batch 1; at 96 and 160 knots "pcg_rpl" / "pcg_lqk" = 1 and "pcg_lpk" = 1 are refused):
  "defaults": per key [rc, value] of mpcg_get_option on a fresh handle (value null when the get failed) — mpcg_create's choices of "pcg_waves"
              and friends included; "cluster_fixups" and "symmetry_state" of a handle that has solved nothing;
  "set":      per key and per value of VALUES, on a fresh handle each: [rc of set, mpcg_last_error when the set failed else null,
              rc of the get afterwards, its value (null when the get failed), "auto_cfg" afterwards].
KEYS is written out literally — every key of either function plus one unknown key — so a key the library drops fails the test."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "option_table.json")

KNOTS = (8, 96, 160)
VALUES = (-2, -1, 0, 1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65, 2048, 2049)
KEYS = (
    # the launch knobs of the single-workgroup kernels and the kernel-family switches
    "pcg_waves", "pcg_max_wg_per_cu", "pcg_reg_rows", "pcg_lds_rows", "pcg_stream_bufs", "lds_extra",
    "pcg16_waves", "pcg16_reg_rows", "pcg16_lds_rows",
    "pcg_rpl", "rpl_waves", "pcg_lqk", "pcg_lqb", "pcg_lpk", "pcg_resident",
    "cluster", "cluster_fixup", "cluster_l2", "cluster_test_fail", "cluster_fixups", "reserve_f64",
    "nt_loads", "sched_hint", "spmv_mfma", "spmv_blocks_per_cu",
    # the symmetry latch
    "check_symmetry", "assume_symmetric", "symmetry_state", "last_symmetry_violations",
    # producers and plant
    "schur_dpp", "schur_chunk", "last_schur_chunk", "dz_dpp", "last_dz_route", "producers_generic",
    "block_solve_wide", "block_solve_f64", "kkt_analytic", "kkt_f32", "merit_f32", "integrator", "sim_integrator",
    # read-only facts
    "num_cus", "auto_cfg",
    "last_kernel_family", "last_kernel_waves", "last_kernel_reg_rows", "last_kernel_lds_rows", "last_kernel_lds_extra",
    "last_kernel_stream_bufs", "last_kernel_cluster", "last_kernel_lds_bytes",
    "no_such_option",
)


def _get(lib, h, key):
    v = C.c_int(-12345)
    rc = lib.mpcg_get_option(h, key.encode(), C.byref(v))
    return [rc, v.value if rc == 0 else None]


def record():
    """The table as a dict (what main() writes)."""
    import torch
    from mpcgpu_amd import _lib
    lib = _lib.load()
    dev = torch.cuda.current_device()

    def fresh(N):
        h = C.c_void_p()
        assert lib.mpcg_create(C.byref(h), dev, 14, N, 1) == 0, lib.mpcg_last_error(None)
        return h

    table = {"knots": list(KNOTS), "values": list(VALUES), "keys": list(KEYS), "handles": {}}
    for N in KNOTS:
        h = fresh(N)
        defaults = {key: _get(lib, h, key) for key in KEYS}
        lib.mpcg_destroy(h)
        sets = {}
        for key in KEYS:
            row = {}
            for v in VALUES:
                h = fresh(N)
                rc = lib.mpcg_set_option(h, key.encode(), v)
                err = lib.mpcg_last_error(h).decode() if rc != 0 else None
                row[str(v)] = [rc, err] + _get(lib, h, key) + [_get(lib, h, "auto_cfg")[1]]
                lib.mpcg_destroy(h)
            sets[key] = row
        table["handles"][f"N{N}"] = {"defaults": defaults, "set": sets}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--force", action="store_true", help="overwrite an existing table")
    args = ap.parse_args()
    if os.path.exists(args.out) and not args.force:
        sys.exit(f"{args.out} exists: the table is a record of the library before a change — pass --force to replace it")
    table = record()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, separators=(",", ":"), sort_keys=False)
        f.write("\n")
    print(f"{len(KEYS)} keys x {len(VALUES)} values x {len(KNOTS)} handles -> {args.out} ({os.path.getsize(args.out)} bytes)")


if __name__ == "__main__":
    main()
