"""`python bench.py --gpus N` must start the ranks itself: fresh child processes, rendezvous env, rc propagation,
and no GPU call in the parent.  CPU-only: the children here are probe scripts, not the bench."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _probe(tmp_path, body):
    p = tmp_path / "probe.py"
    p.write_text(textwrap.dedent(body))
    return str(p)


def test_launcher_spawns_ranks_with_rendezvous_env(tmp_path, monkeypatch):
    monkeypatch.setenv("WF_SHARE_GPU", "1")  # no GPUs in this container: skip the device-count check
    out = tmp_path / "out"
    out.mkdir()
    script = _probe(tmp_path, f"""
        import json, os, sys
        keys = ["RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "HSA_ENABLE_IPC_MODE_LEGACY"]
        json.dump({{k: os.environ.get(k) for k in keys}} | {{"argv": sys.argv[1:]}}, open(os.path.join({str(out)!r}, os.environ["RANK"]), "w"))
    """)
    rc = bench.launch_ranks(3, ["--gpus", "3", "--steps", "2"], script=script)
    assert rc == 0
    recs = [json.load(open(out / str(r))) for r in range(3)]
    assert [r["RANK"] for r in recs] == ["0", "1", "2"] and [r["LOCAL_RANK"] for r in recs] == ["0", "1", "2"]
    assert all(r["WORLD_SIZE"] == "3" and r["MASTER_ADDR"] == "127.0.0.1" for r in recs)
    assert len({r["MASTER_PORT"] for r in recs}) == 1 and all(r["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" for r in recs)
    assert all(r["argv"] == ["--gpus", "3", "--steps", "2"] for r in recs)


def test_launcher_propagates_failure_and_stops_the_other_ranks(tmp_path, monkeypatch):
    monkeypatch.setenv("WF_SHARE_GPU", "1")
    script = _probe(tmp_path, """
        import os, sys, time
        if os.environ["RANK"] == "1":
            sys.exit(7)
        time.sleep(60)  # a surviving rank would wait in a collective for ever
    """)
    import time
    t0 = time.time()
    rc = bench.launch_ranks(2, [], script=script)
    assert rc == 7 and time.time() - t0 < 30


def test_launcher_refuses_more_ranks_than_gpus(monkeypatch):
    monkeypatch.delenv("WF_SHARE_GPU", raising=False)
    assert bench.launch_ranks(64, []) == 2


def test_main_becomes_launcher_before_any_gpu_call(monkeypatch):
    import torch

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = {}
    monkeypatch.setattr(bench, "launch_ranks", lambda n, argv, script=None, budget_s=None: seen.update(n=n, argv=list(argv)) or 0)

    def boom(*a, **k):
        raise AssertionError("the launcher parent touched the GPU")

    monkeypatch.setattr(torch.cuda, "set_device", boom)
    monkeypatch.setattr(torch.cuda, "init", boom)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "2", "--steps", "2", "--layers", "2"])
    assert e.value.code == 0 and seen == {"n": 2, "argv": ["--gpus", "2", "--steps", "2", "--layers", "2"]}


# ---- the supervised two-attempt launch: a failed or hung first attempt ends in ONE conservative relaunch in fresh processes
_RANK_PROBE = """
    import json, os, sys, time
    sys.path.insert(0, %(root)r)
    import torch
    import bench
    from worldforge_amd import parallel
    bench.claim_stdout()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    attempt = int(os.environ["WF_BENCH_ATTEMPT"])
    conservative = "--conservative" in sys.argv
    assert (attempt == 2) == conservative and (("--exchange" in sys.argv) == conservative)
    comm = parallel.init(world, rank, 0)                       # gloo, through the supervisor's store behind the attempt's prefix
    comm.halo_whole_job = conservative
    groups = comm.prepare(cfg_groups=0 if conservative else 2, halo_distances=() if conservative else parallel.halo_distances(world))
    inject = os.environ.get("WF_TEST_INJECT", "")
    if attempt == 1 and inject == "fail" and rank == 2:
        print("rank 2: injected RCCL refusal", file=sys.stderr, flush=True)
        sys.exit(3)
    if attempt == 1 and inject == "hang" and rank == 1:
        print("rank 1: injected hang", file=sys.stderr, flush=True)
        time.sleep(600)
    # a halo exchange and a job all-gather through the prepared groups
    top, bottom = torch.full((3,), float(rank)), torch.full((3,), float(rank) + 0.5)
    up, down = comm.neighbor_rows(top, bottom, 1)
    assert (up is None) == (rank == 0) and (down is None) == (rank == world - 1)
    assert up is None or float(up[0]) == rank - 1 + 0.5
    assert down is None or float(down[0]) == rank + 1
    up2, down2 = comm.neighbor_rows(top, bottom, 2)
    assert (up2 is None) == (rank < 2) and (up2 is None or float(up2[0]) == rank - 2 + 0.5)
    out = torch.empty((world, 1))
    comm.all_gather(out, torch.tensor([float(rank)]))
    comm.barrier()
    if rank == 0:
        bench.emit_json({"metric": "probe", "value": float(out.sum()), "attempt": attempt, "groups": len(groups),
                         "kinds": sorted({k for k, _ in groups}), "collectives_used": sorted(comm.used), "rccl": parallel.rccl_info()})
    bench.shutdown_comm()
"""


def _run_supervised(tmp_path, monkeypatch, inject, budget_s):
    monkeypatch.setenv("WF_SHARE_GPU", "1")
    monkeypatch.setenv("WF_COMM_BACKEND", "gloo")
    monkeypatch.setenv("WF_TEST_INJECT", inject)
    script = _probe(tmp_path, _RANK_PROBE % {"root": ROOT})
    code = ("import sys; sys.path.insert(0, %r); import bench; sys.exit(bench.launch_ranks(4, ['--gpus', '4'], script=%r, budget_s=%r))"
            % (ROOT, script, budget_s))
    return subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)


def test_supervisor_clean_first_attempt_prints_one_line_without_fallback(tmp_path, monkeypatch):
    r = _run_supervised(tmp_path, monkeypatch, "", 300.0)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] == 6.0 and d["attempt"] == 1 and "fallback" not in d
    # world + 2 CFG groups + pair groups at distances 1 and 2 of 4 ranks (3 + 2), every one created in Comm.prepare
    assert d["groups"] == 1 + 2 + 3 + 2 and d["kinds"] == ["cfg", "halo1", "halo2", "world"]
    assert d["collectives_used"] == ["all_gather", "barrier"] and d["rccl"]["world"] == 4 and d["rccl"]["backend"] == "gloo"


@pytest.mark.parametrize("inject,budget_s,reason", [("fail", 300.0, "rank 2 exited with code 3"), ("hang", 25.0, "wall budget of 25 s exceeded")])
def test_supervisor_relaunches_conservatively_after_a_failure_or_a_hang(tmp_path, monkeypatch, inject, budget_s, reason):
    """World-4 gloo ranks through the real launcher: attempt 1 loses rank 2 (non-zero exit) or hangs on rank 1 until the wall budget;
    every rank of it is stopped, and attempt 2 runs in fresh processes with `--exchange gather --conservative` (no process group beyond
    the job's own: the halo rows travel by the whole-job all-gather) and labels its line."""
    r = _run_supervised(tmp_path, monkeypatch, inject, budget_s)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout                      # attempt 1 never reaches stdout
    d = json.loads(lines[0])
    assert d["fallback"] is True and d["attempt"] == 2 and d["value"] == 6.0
    assert reason in d["first_attempt"]["reason"]
    assert any("injected" in ln for ln in d["first_attempt"]["stderr_tail"])
    assert d["groups"] == 1 and d["kinds"] == ["world"]    # conservative: nothing but the job's own communicator
    assert "ONE relaunch in fresh processes" in r.stderr


def test_supervisor_killed_by_its_launcher_takes_its_ranks_with_it(tmp_path, monkeypatch):
    """A launcher that gives up sends SIGTERM: the supervisor must not leave rank processes behind (on a real node they would hold the
    GPUs and wedge the next run)."""
    import signal
    import time
    monkeypatch.setenv("WF_SHARE_GPU", "1")
    pidfile = tmp_path / "pids"
    script = _probe(tmp_path, f"""
        import os, time
        open({str(pidfile)!r}, "a").write(str(os.getpid()) + "\\n")
        time.sleep(600)
    """)
    code = ("import sys; sys.path.insert(0, %r); import bench; sys.exit(bench.launch_ranks(2, [], script=%r, budget_s=500.0))" % (ROOT, script))
    sup = subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    t0 = time.time()
    while time.time() - t0 < 120 and (not pidfile.exists() or len(pidfile.read_text().split()) < 2):
        time.sleep(0.2)
    pids = [int(x) for x in pidfile.read_text().split()]
    assert len(pids) == 2
    sup.send_signal(signal.SIGTERM)
    sup.wait(timeout=60)
    time.sleep(1.0)
    for pid in pids:
        try:
            os.kill(pid, 0)
            alive = open(f"/proc/{pid}/status").read().split("State:")[1].split()[0] != "Z"
        except (ProcessLookupError, FileNotFoundError):
            alive = False
        assert not alive, f"rank process {pid} survived its supervisor"


def test_supervisor_under_torch_distributed_run(tmp_path, monkeypatch):
    """The driver's N > 1 command starts the ranks with torch.distributed.run: each of its workers then supervises the real rank as a
    child and the supervisors agree through the launcher's own store (bench.supervise_under_launcher)."""
    monkeypatch.setenv("WF_SHARE_GPU", "1")
    monkeypatch.setenv("WF_COMM_BACKEND", "gloo")
    monkeypatch.setenv("WF_TEST_INJECT", "fail")
    body = ("import os, sys\nsys.path.insert(0, %r)\nif not os.environ.get('WF_BENCH_CHILD'):\n    import bench\n"
            "    sys.exit(bench.supervise_under_launcher(sys.argv[1:], script=os.path.abspath(__file__), budget_s=300.0))\n" % ROOT
            + textwrap.dedent(_RANK_PROBE % {"root": ROOT}))
    p = tmp_path / "probe_tr.py"
    p.write_text(body)
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(p), "--gpus", "4"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["fallback"] is True and d["attempt"] == 2 and d["value"] == 6.0 and "rank 2 exited with code 3" in d["first_attempt"]["reason"]


def test_world_size_must_match_gpus(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "4")
    ns = type("A", (), {"gpus": 2})
    with pytest.raises(SystemExit):
        bench.rank_env(ns)


def test_stdout_carries_only_the_json_line():
    """RCCL prints a version banner on the C-level stdout of a rank (flushed at exit, after the result line): bench.claim_stdout() keeps
    fd 1 for the JSON line alone and sends every other writer -- Python prints, C stdio, child processes -- to stderr."""
    code = ("import os, sys, ctypes; sys.path.insert(0, %r); import bench; bench.claim_stdout(); bench.claim_stdout();"
            "print('python chatter'); libc = ctypes.CDLL(None); libc.puts(b'C stdio banner'); os.system('echo child chatter');"
            "bench.emit_json({'metric': 'x', 'value': 1.5})") % ROOT
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == '{"metric": "x", "value": 1.5}\n'
    for noise in ("python chatter", "C stdio banner", "child chatter"):
        assert noise in r.stderr


def test_comm_probe_parses_rccl_logs_and_gpu_count_needs_no_hip(tmp_path, monkeypatch):
    """tools/comm_probe.py: the RCCL log summary (channels / AllGather tuning lines), and bench.visible_gpu_count(), which the launchers use
    instead of torch.cuda.device_count() so that the parent never initialises HIP."""
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    probe = importlib.import_module("comm_probe")
    log = tmp_path / "rccl.log"
    log.write_text("host:1:1 [0] NCCL INFO RCCL version 2.26.6-HEAD:64f48b6\n"
                   "host:1:1 [0] NCCL INFO Channel 00/32 :    0   1   2   3   4   5   6   7\n"
                   "host:1:1 [0] NCCL INFO Channel 31/32 :    0   7   6   5   4   3   2   1\n"
                   "host:1:1 [0] NCCL INFO AllGather: 83886080 Bytes -> Algo 1 proto 2 time 612.5\n"
                   "host:1:1 [0] NCCL INFO AllGather: 83886080 Bytes -> Algo 1 proto 2 time 612.5\n")
    r = probe.rccl_log_summary(str(log))
    assert r["channels"] == 32 and r["version"].startswith("RCCL version 2.26") and len(r["tuning"]) == 1 and "Algo 1" in r["tuning"][0]
    assert probe.rccl_log_summary(str(tmp_path / "missing.log"))["channels"] is None
    import bench
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1,2,5")
    assert bench.visible_gpu_count() == 4
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    assert bench.visible_gpu_count() == 0
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    for v in ("ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(v, raising=False)
    n = bench.visible_gpu_count()          # from /sys/class/kfd (None where that is unreadable, 0 in a GPU-less container)
    assert n is None or n >= 0


def test_exchange_calibration_picks_by_extrapolated_time_and_keeps_the_default_on_ties(monkeypatch):
    """bench.calibrate_exchange (N > 1 runs, before the timed window): times every candidate on a model cut to 4 and to 12 layers, extrapolates
    linearly to the full depth (a candidate with a large per-forward fixed cost but a cheap layer must win against one that looks better at 4
    layers), keeps the FIRST candidate unless another is >= 3 % faster, drops a candidate whose host side refuses the shape (never the
    default), switches the model's communicator / the pipeline's CFG branch for the `cfg2+` candidates, and reports every estimate."""
    import time
    import types

    import torch

    import bench

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)

    class FakeComm:
        def __init__(self, world, group_index=0):
            self.world, self.group_index = world, group_index

        def barrier(self):
            pass

        def all_reduce_max(self, t):
            return t

    world, sub = FakeComm(8), FakeComm(4, group_index=1)
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(num_layers=40), comm=world, _ws={("kvx", 1): object(), ("x", 2): object()},
                                  pair_lockstep=None, exchange_mode=None, exchange_chunks=None)
    pipe = types.SimpleNamespace(cfg_split=None)
    ctx = {"world": world, "sub": sub, "pipe": pipe}
    # per-candidate cost model in ms: fixed + per-layer * depth
    cost = {"lockstep": (2.0, 1.00), "chunked2": (2.0, 1.02), "cfg2+chunked2": (6.0, 0.80), "bcast": (0.5, 1.10), "gather": (2.0, 0.99)}
    seen = []

    def run(name):
        if name == "bcast":
            raise ValueError("this shape is not served")
        seen.append((name, model.cfg.num_layers, model.comm is sub, pipe.cfg_split))
        fixed, per = cost[name]
        time.sleep((fixed + per * model.cfg.num_layers) * 1e-3)

    out = bench.calibrate_exchange(model, world, run, list(cost), "num_layers", torch.device("cpu"), "auto", reps=2, ctx=ctx)
    assert model.cfg.num_layers == 40 and ("kvx", 1) not in model._ws and ("x", 2) in model._ws
    assert set(out["dropped"]) == {"bcast"} and "bcast" not in out["estimated_ms_per_evaluation"]
    est = out["estimated_ms_per_evaluation"]
    # at 4 layers cfg2+chunked2 (6 + 3.2 = 9.2 ms) looks WORSE than lockstep (6.0 ms); extrapolated to 40 layers it wins (38 vs 42 ms)
    assert out["timed_ms"]["cfg2+chunked2"]["4"] > out["timed_ms"]["lockstep"]["4"]
    assert est["cfg2+chunked2"] < 0.97 * est["lockstep"] and out["selected"] == "cfg2+chunked2"
    assert model.comm is sub and pipe.cfg_split == (world, 1) and (model.pair_lockstep, model.exchange_mode, model.exchange_chunks) == (False, "chunked", 2)
    assert any(s[0] == "cfg2+chunked2" and s[2] and s[3] == (world, 1) for s in seen) and all(not s[2] and s[3] is None for s in seen if s[0] == "lockstep")
    # `gather` is ~1 % faster than the default: inside the 3 % band -> the default stays
    cost.pop("cfg2+chunked2")
    model.comm, pipe.cfg_split = world, None
    out2 = bench.calibrate_exchange(model, world, run, ["lockstep", "chunked2", "gather"], "num_layers", torch.device("cpu"), "auto", reps=2, ctx=ctx)
    assert out2["selected"] == "lockstep" and model.comm is world and pipe.cfg_split is None and model.pair_lockstep is True
    # forced
    out3 = bench.calibrate_exchange(model, world, run, ["lockstep"], "num_layers", torch.device("cpu"), "cfg2+gather", ctx=ctx)
    assert out3["selected"] == "cfg2+gather" and model.comm is sub and model.exchange_mode == "gather"


def test_dump_outputs_writes_float32_and_samples_the_same_elements_over_the_limit(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: what the timed path returned, as DIR/<name>.npy in float32; over the size limit a fixed seeded sample
    of each array, the same indices on every call, so that two builds can be compared element for element."""
    import numpy as np
    import torch

    lat = torch.randn(1, 16, 3, 4, 5, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "a"), {"latents": lat})
    got = np.load(tmp_path / "a" / "latents.npy")
    assert got.dtype == np.float32 and got.shape == tuple(lat.shape)
    np.testing.assert_array_equal(got, lat.float().numpy())

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1024)
    big = torch.arange(4096, dtype=torch.float32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"x": big})
    b, c = np.load(tmp_path / "b" / "x.npy"), np.load(tmp_path / "c" / "x.npy")
    assert b.nbytes <= 1024 and b.size == 256
    np.testing.assert_array_equal(b, c)
    assert np.all(np.diff(b) > 0)                      # sampled values keep their order (here: the element indices themselves)


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--steps", "50"], ["--steps", "45", "--warmup", "6"],
                                  ["--workload", "longcat", "--dump-outputs", "x"]])
def test_bench_refuses_arguments_it_cannot_honour_before_any_gpu_call(argv, monkeypatch):
    import torch

    def boom(*a, **k):
        raise AssertionError("touched the GPU")

    monkeypatch.setattr(torch.cuda, "set_device", boom)
    with pytest.raises(SystemExit) as e:
        bench.main(argv)
    assert e.value.code not in (0, None)


def test_bench_window_times_exactly_steps_inside_the_schedule():
    """--steps K --warmup W: K timed steps after W warm-up steps, max(1, round(0.3 K)) of them guided (schedule steps < 15)."""
    for K in range(1, 50):
        for Wm in range(0, 50 - K):
            s = bench.window_start(K, Wm)
            if s + Wm + K > 50:
                continue
            timed = range(s + Wm, s + Wm + K)
            assert len(timed) == K and timed[-1] < 50
            assert sum(i < 15 for i in timed) == min(K, max(1, round(0.3 * K))) or s == 0
