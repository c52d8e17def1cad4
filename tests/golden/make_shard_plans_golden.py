"""
tests/golden/make_shard_plans_golden.py — the exchange plans of the sharded tests, recorded as data.

Bit-identical results do not pin a plan: a different split of a shard into swept-first and interior parts, other
destination masks or another exchange mode can all be correct.  This script records what the planner (pi_exchange_plan,
csrc/pi_comm.cpp) decided for every rank of every case of tests/test_gpu_p2p.py::CASES (rank processes over the
peer-to-peer transport) and of tests/test_gpu_endtoend.py::ROW_EXACT_CASES (logical ranks over the in-process
transport, row-exact and coarse), so that a change of the host code that is meant to leave the plans alone can show it
did: the five info[] values, pi_plan_ranges and every plan selector of pi_comm_info (tests/helpers.py: plan_record).

The record in tests/golden/shard_plans.json was taken at commit 3633377 ("Add fused on-device rollouts that switch
between two policies"), the last one before the planner was restructured into named steps.  Run it on a GPU box, from
a built tree, ONLY at a commit whose plans are known to be the wanted ones — never to make a failing comparison pass:

    python -m tests.golden.make_shard_plans_golden
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import threading
import uuid
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

OUT = Path(__file__).resolve().parent / "shard_plans.json"
RECORDED_AT = "3633377"


def p2p_plans() -> dict:
    import torch.multiprocessing as mp
    from dynamicprogramming_amd import envs
    from tests import helpers as H
    from tests.test_gpu_p2p import CASES, _free_port, _worker
    plans = {}
    for world, name, shape, mode, extra in CASES:
        env = {"PI_MI355_EXCHANGE": mode, **extra}
        key = H.plan_key("p2p", world, name, shape, env)
        if key in plans:                                    # the same plan again, poisoned
            continue
        cfg_kw = {**envs.ENVS[name].CONFIG, "max_pi_iter": 3, "max_eval_iter": 60}
        with tempfile.TemporaryDirectory(prefix="shard_plans_") as tmp:
            mp.spawn(_worker, args=(world, _free_port(), name, shape, cfg_kw, tmp, {**env, "TEST_PLAN_ONLY": "1"}),
                     nprocs=world, join=True)
            plans[key] = [json.loads((Path(tmp) / f"rank{r}_plan.json").read_text()) for r in range(world)]
        print(f"{key}: {world} ranks", flush=True)
    return plans


def local_plans() -> dict:
    import torch
    from dynamicprogramming_amd import envs
    from dynamicprogramming_amd import transport as T
    from tests import helpers as H
    from tests.test_gpu_endtoend import ROW_EXACT_CASES
    plans = {}
    for world, name, shape in ROW_EXACT_CASES:
        cls = envs.ENVS[name]
        for row_exact in ("1", "0"):
            env = {"PI_MI355_EXCHANGE": "halo", "PI_MI355_ROW_EXACT": row_exact}
            os.environ.update(env)
            group = f"plans-{uuid.uuid4().hex}"
            out, errors = [None] * world, []

            def rank_main(r):
                try:
                    with torch.cuda.stream(torch.cuda.Stream(device="cuda:0")):
                        s = cls(H.env_bins_space(name, shape), cls.ACTIONS, envs.CudaPIConfig(**cls.CONFIG), device="cuda:0",
                                transport=T.NativeTransport.local(r, world, group))
                        out[r] = H.plan_record(s._backend.engine, dict(s._comm.info))
                        torch.cuda.synchronize()
                        s._backend.close()
                except Exception as exc:  # noqa: BLE001
                    errors.append((r, repr(exc)))

            threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
            for t in threads:
                t.start()
            for t in threads:
                t.join(timeout=300)
            if errors or any(o is None for o in out):
                raise SystemExit(f"{name} {shape} world {world}: {errors}")
            key = H.plan_key("local", world, name, shape, env)
            plans[key] = out
            print(f"{key}: {world} ranks", flush=True)
    return plans


def main() -> None:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("the plans are made by the library on a GPU: run this on a GPU box")
    plans = {**p2p_plans(), **local_plans()}
    body = ",\n".join(f"{json.dumps(k)}: {json.dumps(plans[k], sort_keys=True)}" for k in sorted(plans))     # a case a line
    OUT.write_text(f'{{"recorded_at": "{RECORDED_AT}", "plans": {{\n{body}\n}}}}\n')
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, {len(plans)} cases)")


if __name__ == "__main__":
    main()
