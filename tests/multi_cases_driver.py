"""One case of tests/multi_inputs.py through cd_multi_step on ONE GPU, as tests/multi_loopback_driver.py runs its cloth shards: every
rank is a host thread of this process with a context of its own, and libmi355cd.so talks to tests/loopback_rccl (selected through
MI355CD_RCCL_LIBRARY) instead of RCCL.  Run as a child process by tests/test_multi_step_gpu.py.

usage: multi_cases_driver.py CASE

Every run of the case goes through its schedule: before a step a rank sets the CD_MULTI_* flags and uploads the vertices the schedule
gives it, then steps into a buffer of its own with multi_inputs.CANARY in the rows behind cap (or with a NULL pointer).  Every step is
judged by multi_inputs.compare against the oracle on the merged mesh of that step.  Prints ONE JSON line -- per run and step the checks
and what the step reported of itself (host_syncs, attempts, the timing fields, cd_stats.stack_overflows, the sort's form) -- and exits
non-zero when a check failed.  Threads are joined with a time-out: one still alive then is reported (ok: false) and the process leaves
through os._exit, as the cloth driver does."""
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
os.environ["MI355CD_RCCL_LIBRARY"] = os.path.join(HERE, "loopback_rccl", "librccl_loopback.so")
import torch  # noqa: F401,E402  (its HIP runtime first, see conftest.py)
sys.path[:0] = [os.path.join(ROOT, "gpu-computing-course_amd", "pyhost"), HERE]
import numpy as np  # noqa: E402
import mi355cd  # noqa: E402
import multi_inputs as mu  # noqa: E402

JOIN_SECONDS = 60
MS = ("ms_tree", "ms_allgather", "ms_pack", "ms_counts", "ms_exchange", "ms_local", "ms_cross")


def run_one(name, run_index, run):
    W = len(run.ranks)
    cds = []
    for rk in run.ranks:
        cd = mi355cd.CollisionDetector(rk.verts, rk.vidx, rk.ids)
        for key, value in rk.options.items():
            if key == "frame":
                cd.set_morton_frame(*value)
            else:
                cd.set_option(key, value)
        cd.set_vertex_id_base(rk.vbase)
        cds.append(cd)
    uid = mi355cd.multi_unique_id()                 # also loads the loopback library once, before the threads start
    assert uid[8:16] == b"loopback", "libmi355cd.so did not load the loopback library"
    results, errors = [None] * W, [None] * W

    def rank_main(r):
        try:
            with mi355cd.MultiStep(cds[r], uid, r, W, query_cap_per_peer=run.qcap, flags=run.create_flags) as ms:
                out = []
                for st in run.steps:
                    if st.flags is not None and st.flags[r] is not None:
                        ms.set_flags(st.flags[r])
                    if st.updates is not None and st.updates[r] is not None:
                        cds[r].update_vertices(st.updates[r])
                    cap = run.cap if st.caps is None or st.caps[r] is None else st.caps[r]
                    null = bool(st.null and st.null[r])
                    buf = None if null else np.full((cap + mu.CANARY_ROWS, 2), mu.CANARY, dtype=np.uint32)
                    _, n, rc, info = ms.step(cap=cap, pairs=buf)
                    out.append(dict(pairs=buf, cap=cap, null=null, n=n, rc=rc, info={k: getattr(info, k) for k, _ in info._fields_},
                                    stack_overflows=int(cds[r].stats().stack_overflows), sort_form=int(cds[r].debug_get(mi355cd.CD_DBG_GET_SORT_FORM)),
                                    root=cds[r].root_box()))
                results[r] = out
        except BaseException as e:                  # noqa: BLE001
            errors[r] = repr(e)

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(W)]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN_SECONDS)
    hung = [r for r, t in enumerate(th) if t.is_alive()]
    if hung or any(errors):
        print(json.dumps({"ok": False, "case": name, "run": run.name, "hung": hung, "errors": errors}))
        sys.stdout.flush()
        os._exit(2)
    ids_of_rank = [rk.ids for rk in run.ranks]
    steps = []
    for it in range(len(run.steps)):
        want = mu.want(name, run_index, it)
        res = [results[r][it] for r in range(W)]
        checks = mu.compare(want, res, ids_of_rank)
        checks["root_box_is_the_box_of_the_vertices"] = all(np.array_equal(np.asarray(x["root"], dtype=np.float64), want.roots[r]) for r, x in enumerate(res))
        infos = [x["info"] for x in res]
        steps.append({"checks": checks, "rc": [x["rc"] for x in res], "n": [x["n"] for x in res], "cap": [x["cap"] for x in res],
                      "attempts": [i["attempts"] for i in infos], "query_cap": [i["query_cap"] for i in infos], "host_syncs": [i["host_syncs"] for i in infos],
                      "n_peers": [i["n_peers"] for i in infos], "sent": [i["sent_queries"] for i in infos], "recv": [i["recv_queries"] for i in infos],
                      "local": [i["local_pairs"] for i in infos], "cross": [i["cross_pairs"] for i in infos],
                      "pairs_tested": [i["pairs_tested"] for i in infos], "want_pairs_tested": want.tested,
                      "ms": [{k: float(i[k]) for k in MS} for i in infos], "stack_overflows": [x["stack_overflows"] for x in res],
                      "sort_form": [x["sort_form"] for x in res], "want_pairs": int(want.pairs.size)})
    for cd in cds:
        cd.close()
    return {"run": run.name, "steps": steps, "ok": all(all(bool(v) for v in s["checks"].values()) for s in steps)}


def main():
    name = sys.argv[1]
    case = mu.case(name)
    runs = [run_one(name, k, run) for k, run in enumerate(case.runs)]
    ok = all(r["ok"] for r in runs)
    print(json.dumps({"ok": ok, "case": name, "world": case.world, "runs": runs}, default=lambda o: bool(o) if isinstance(o, np.bool_) else int(o)))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
