"""Recorder of tests/golden/lds_vectors_parent.npz, the fixture of tests/test_lds_vectors.py (needs a GPU).

Run it on a build of the PARENT commit's solver (VBOC_LIB=<that build inside the repository>): the fixture pins the
results of the commit before the sweeps' per-stage vectors moved from the stage record into LDS rows, and the test
compares the product library with it bit for bit.  The file carries the inputs themselves (so no host's numpy decides
them) and, of the outputs, status / sqp_iter / qp_iter / cost / x_0 in full and the sha1 of x and u:

  in_<key>      the ragged wave-solver batch: 4 problems per horizon of HORIZONS, ids 4j .. 4j+3 from
                data_generation_ics(3, ids, N=N), guesses padded to nmax = 120
  out_<key>     solve_host of that batch (wave_all = 1, nlp_solver_max_iter = 200): k_wave<3, true>
  dg_* / ts_*   the device data-generation loop (k_dg<3, true>) and the device testing loop (k_ts<3, true>) on
                DG_IDS: per problem the row count and the rows, concatenated
  dg<S>_* / ts<S>_*   the same loops started at the horizon S of DG_STARTS (a problem's solves run at S .. S + 9 and
                its verification solves up to S + 12), so that the two kernels meet the ragged batch's horizons:
                2 .. 14 (partial, one and two 3-stage groups), 51 .. 64 (the stage-parallel trips full at 63,
                spilling one lane at 64) and 108 .. 120 (the last rows and the top group's over-read)
  dg1_* / ts1_* the loops at SEQ_START on ONE workgroup (wave_groups = 1, no speculative or parked jobs): every
                problem's short first solves follow the previous problem's longest ones on the same LDS rows

usage: VBOC_LIB=$PWD/vboc_amd/variants/libvboc_amd_parent.so python tools/record_lds_vectors.py [--out file.npz]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HORIZONS = (2, 3, 4, 5, 7, 8, 63, 64, 100, 112, 119, 120)
PER = 4
NMAX = 120
MAX_ITER = 200
DG_IDS = 12
DG_STARTS = (2, 3, 5, 51, 63, 108)
START_IDS, START_TS_IDS = 6, 4
SEQ_START, SEQ_IDS = 108, 4
IN_KEYS = ("N", "x_guess", "u_guess", "p", "lbx", "ubx", "lbu", "ubu", "lbx0", "ubx0", "lbxe", "ubxe")
OUT_KEYS = ("status", "sqp_iter", "qp_iter", "cost", "x", "u")


def ragged_batch():
    from vboc_amd.ics import data_generation_ics
    parts = [data_generation_ics(3, np.arange(PER * j, PER * j + PER), N=N) for j, N in enumerate(HORIZONS)]
    b = {}
    for k in IN_KEYS:
        arrs = []
        for p in parts:
            a = np.asarray(p[k])
            if k == "x_guess":
                a = np.concatenate([a, np.repeat(a[:, -1:], NMAX + 1 - a.shape[1], 1)], 1)
            if k == "u_guess":
                a = np.concatenate([a, np.zeros((a.shape[0], NMAX - a.shape[1], a.shape[2]))], 1)
            arrs.append(a)
        b[k] = np.ascontiguousarray(np.concatenate(arrs))
    return b


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def solve(b, **opts):
    from vboc_amd import lib
    s = lib.Solver(3, NMAX, slots=opts.pop("slots", 1024))
    for k, v in opts.items():
        s.set_option(k, v)
    try:
        g = s.solve_host(b)
        g["last_groups"] = s.get_option("last_groups")
        return g
    finally:
        s.close()


def flat_rows(results, ncols):
    """Per-problem results (a list of samples, one array, or None) as (counts, rows)."""
    cnt, rows = [], []
    for r in results:
        a = np.zeros((0, ncols)) if r is None else np.asarray(r, dtype=np.float64).reshape(-1, ncols)
        cnt.append(-1 if r is None else a.shape[0])
        rows.append(a)
    return np.array(cnt, dtype=np.int64), np.concatenate(rows)


def device_loops(tag="", dg_ids=None, ts_ids=None, N_start=None, **opts):
    """The two device loops on a fresh Solver(3, NMAX) with `opts` set; keys dg<tag>_* / ts<tag>_*."""
    from vboc_amd import lib
    from vboc_amd.drivers import data_generation_device, testing_device
    dg_ids = np.arange(DG_IDS) if dg_ids is None else np.asarray(dg_ids)
    ts_ids = dg_ids if ts_ids is None else np.asarray(ts_ids)
    s = lib.Solver(3, NMAX)
    for k, v in opts.items():
        s.set_option(k, v)
    try:
        dg, dst = data_generation_device(3, dg_ids, s, N_start=N_start)
        groups = s.get_option("last_groups")
        ts, tst = testing_device(3, ts_ids, s, N_start=N_start)
    finally:
        s.close()
    dgc, dgr = flat_rows(dg, 6)
    tsc, tsr = flat_rows(ts, 6)
    # per problem: OCP solves, twin steps, SQP iterations (schedule-independent counts)
    return {f"dg{tag}_cnt": dgc, f"dg{tag}_rows": dgr, f"dg{tag}_counts": np.asarray(dst["per_problem"])[:, :3].copy(),
            f"ts{tag}_cnt": tsc, f"ts{tag}_rows": tsr, f"ts{tag}_counts": np.asarray(tst["per_problem"])[:, :3].copy(),
            f"dg{tag}_groups": np.array(int(groups))}


def start_loops(S):
    """The loops started at horizon S: ids of their own per start."""
    j = DG_STARTS.index(S)
    return device_loops(str(S), np.arange(100 + 8 * j, 100 + 8 * j + START_IDS),
                        np.arange(100 + 8 * j, 100 + 8 * j + START_TS_IDS), N_start=S)


def one_workgroup_loops():
    """The loops at SEQ_START with one workgroup taking the problems one after the other."""
    ids = np.arange(200, 200 + SEQ_IDS)
    return device_loops("1", ids, ids, N_start=SEQ_START, wave_groups=1, dg_speculate=0, dg_park=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lds_vectors_parent.npz"))
    a = ap.parse_args()
    import torch   # before the solver library is loaded: torch brings its own HIP runtime
    assert torch.cuda.is_available(), "the recorder needs a GPU"
    b = ragged_batch()
    g = solve(b, nlp_solver_max_iter=MAX_ITER, coop_threshold=8192, wave_all=1)
    rec = {"in_" + k: b[k] for k in IN_KEYS}
    for k in ("status", "sqp_iter", "qp_iter", "cost"):
        rec["out_" + k] = np.asarray(g[k])
    rec["out_x0"] = np.asarray(g["x"])[:, 0, :]
    rec["out_x_sha1"] = np.array(sha1(g["x"]))
    rec["out_u_sha1"] = np.array(sha1(g["u"]))
    rec.update(device_loops())
    for S in DG_STARTS:
        rec.update(start_loops(S))
    rec.update(one_workgroup_loops())
    rec = {k: v for k, v in rec.items() if not k.endswith("_groups")}
    rec["lib"] = np.array(os.path.basename(os.environ.get("VBOC_LIB") or "libvboc_amd.so"))
    np.savez_compressed(a.out, **rec)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, status {np.bincount(rec['out_status'], minlength=5)}, "
          f"dg rows {rec['dg_rows'].shape}, ts rows {rec['ts_rows'].shape}")
    for tag in [str(S) for S in DG_STARTS] + ["1"]:
        print(f"start {tag}: dg row counts {rec[f'dg{tag}_cnt'].tolist()} solves {rec[f'dg{tag}_counts'][:, 0].tolist()} "
              f"ts row counts {rec[f'ts{tag}_cnt'].tolist()} solves {rec[f'ts{tag}_counts'][:, 0].tolist()}")


if __name__ == "__main__":
    main()
