"""bench.py --gpus N: the attempts it would run as fresh child processes (dry run: nothing touches a GPU), and the
launcher's bookkeeping with children that are not GPU programs at all."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dry(args, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "OMP_NUM_THREADS")}
    env["FROG_BENCH_LAUNCH_DRY_RUN"] = "1"
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    return r


def test_gpus_n_becomes_attempts_of_n_fresh_children():
    r = _dry(["--gpus", "4", "--steps", "20", "--warmup", "5"])
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ranks"] == [0, 1, 2, 3]
    hosts = [(a["host"], a["transport"]) for a in out["attempts"]]
    assert hosts == [("preflight", "rccl"), ("native", "rccl"), ("torch", "nccl")]
    for i, a in enumerate(out["attempts"]):
        cmd = a["command"]
        assert cmd[0] == sys.executable and cmd[1] == os.path.join(ROOT, "bench.py")
        assert cmd[2:8] == ["--gpus", "4", "--steps", "20", "--warmup", "5"]          # the caller's arguments, unchanged
        assert cmd[cmd.index("--child") + 1] == a["host"] and cmd[cmd.index("--child-attempt") + 1] == str(i)


def test_rehearsal_backend_and_host_selection():
    r = _dry(["--gpus", "2"], {"FROG_BENCH_BACKEND": "gloo", "FROG_BENCH_HOSTS": "native"})
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert [(a["host"], a["transport"]) for a in out["attempts"]] == [("native", "shm")]


def test_a_rank_of_a_launched_run_checks_its_world_size():
    # WORLD_SIZE set (what torch.distributed.run gives its children) and --gpus disagreeing: an error, not a launch
    r = _dry(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_the_launcher_is_importable_without_torch_or_the_device_library():
    code = ("import sys, json; sys.path.insert(0, %r); import bench; "
            "assert 'torch' not in sys.modules and 'frog_amd' not in sys.modules; "
            "print(json.dumps(bench.child_command(['--gpus', '2'], 'native', 'rccl', '/tmp/x', 1)))" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    cmd = json.loads(r.stdout)
    assert cmd[-8:] == ["--child", "native", "--child-transport", "rccl", "--child-dir", "/tmp/x", "--child-attempt", "1"]


def test_orchestrator_with_failing_and_hanging_children(tmp_path, monkeypatch):
    """The launcher's bookkeeping on children that never touch a GPU: a preflight that fails puts the host-staged attempt
    in the queue and skips the RCCL ones; a child that hangs is killed at its time-out and reported with its stderr; the
    line that comes out carries every attempt."""
    sys.path.insert(0, ROOT)
    import bench
    fake = tmp_path / "fake_child.py"
    fake.write_text(
        "import json, os, sys, time\n"
        "a = sys.argv; host = a[a.index('--child') + 1]; tr = a[a.index('--child-transport') + 1]\n"
        "rank = int(os.environ['RANK'])\n"
        "if host == 'preflight':\n"
        "    sys.stderr.write('rccl says no\\n'); sys.exit(5)\n"
        "if host == 'native' and tr == 'shm':\n"
        "    if rank == 0: print(json.dumps({'metric': 'm', 'value': 42.0, 'replicas_identical': True}))\n"
        "    sys.exit(0)\n"
        "time.sleep(60)\n")
    monkeypatch.setattr(bench, "child_command", lambda argv, host, tr, d, k: [sys.executable, str(fake), "--child", host, "--child-transport", tr])
    monkeypatch.setenv("FROG_BENCH_PREFLIGHT_TIMEOUT", "20")
    monkeypatch.setenv("FROG_BENCH_ATTEMPT_TIMEOUT", "3")
    monkeypatch.delenv("FROG_BENCH_BACKEND", raising=False)
    monkeypatch.delenv("FROG_BENCH_HOSTS", raising=False)
    import io, contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = bench.orchestrate(None, [], 2, [0, 1], str(tmp_path / "run"))
    assert rc == 0
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    assert line["value"] == 42.0
    tried = line["hosts_tried"]
    assert [(t["host"], t["transport"]) for t in tried] == [("preflight", "rccl"), ("native", "rccl"), ("torch", "nccl"), ("native", "shm")]
    assert tried[0]["ok"] is False and "rccl says no" in tried[0]["stderr_tail"]["0"]
    assert tried[1].get("skipped") and tried[2].get("skipped") and tried[3]["ok"] is True

    # a hang: the RCCL preflight passes, the native attempt never returns
    fake.write_text(
        "import json, os, sys, time\n"
        "a = sys.argv; host = a[a.index('--child') + 1]; tr = a[a.index('--child-transport') + 1]\n"
        "rank = int(os.environ['RANK'])\n"
        "if host == 'preflight':\n"
        "    if rank == 0: print(json.dumps({'preflight': 'rccl', 'known_answers': True, 'latencies_rank0': {}}))\n"
        "    sys.exit(0)\n"
        "if host == 'native' and tr == 'rccl':\n"
        "    sys.stderr.write('stuck in a collective\\n'); sys.stderr.flush(); time.sleep(60)\n"
        "if rank == 0: print(json.dumps({'metric': 'm', 'value': 7.0 if tr == 'shm' else 9.0, 'replicas_identical': True}))\n")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = bench.orchestrate(None, [], 2, [0, 1], str(tmp_path / "run2"))
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    tried = line["hosts_tried"]
    # the native RCCL attempt hung: the other RCCL host is not given the chance to sit out its own time-out, the host-staged
    # transport runs at once
    assert rc == 0 and line["value"] == 7.0
    assert [(t["host"], t["transport"]) for t in tried] == [("preflight", "rccl"), ("native", "rccl"), ("torch", "nccl"), ("native", "shm")]
    assert tried[1]["ok"] is False and tried[1]["return_codes"] == [-9, -9] and tried[1]["timed_out"] is True
    assert "stuck in a collective" in tried[1]["stderr_tail"]["0"] and tried[1]["seconds"] < 10
    assert "hung" in tried[2]["skipped"] and tried[3]["ok"] is True


def test_orchestrator_falls_back_when_every_rccl_attempt_fails_after_a_good_preflight(tmp_path, monkeypatch):
    """Preflight passes, both RCCL hosts fail fast: the host-staged attempt still produces the line."""
    sys.path.insert(0, ROOT)
    import bench
    fake = tmp_path / "fake_child.py"
    fake.write_text(
        "import json, os, sys\n"
        "a = sys.argv; host = a[a.index('--child') + 1]; tr = a[a.index('--child-transport') + 1]\n"
        "rank = int(os.environ['RANK'])\n"
        "if host == 'preflight':\n"
        "    if rank == 0: print(json.dumps({'preflight': 'rccl', 'known_answers': True, 'latencies_rank0': {}}))\n"
        "    sys.exit(0)\n"
        "if tr != 'shm': sys.stderr.write('boom\\n'); sys.exit(3)\n"
        "if rank == 0: print(json.dumps({'metric': 'm', 'value': 5.0, 'replicas_identical': True}))\n")
    monkeypatch.setattr(bench, "child_command", lambda argv, host, tr, d, k: [sys.executable, str(fake), "--child", host, "--child-transport", tr])
    monkeypatch.delenv("FROG_BENCH_BACKEND", raising=False)
    monkeypatch.delenv("FROG_BENCH_HOSTS", raising=False)
    import io, contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = bench.orchestrate(None, [], 2, [0, 1], str(tmp_path / "run"))
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    assert rc == 0 and line["value"] == 5.0
    assert [(t["host"], t["transport"], t["ok"]) for t in line["hosts_tried"]] == [
        ("preflight", "rccl", True), ("native", "rccl", False), ("torch", "nccl", False), ("native", "shm", True)]
    assert "boom" in line["hosts_tried"][1]["stderr_tail"]["0"]


def test_a_failed_rank_stops_the_others_waiting(tmp_path):
    """Rendezvous: a rank that dies before a collective tells the others, who stop waiting at once with its reason."""
    import time
    sys.path.insert(0, ROOT)
    import bench
    a, b = bench.Rendezvous(str(tmp_path), 0, 0, 2), bench.Rendezvous(str(tmp_path), 0, 1, 2)
    b.fail("FrogError: frog_create: device index out of range")
    t0 = time.time()
    try:
        a.all_ready("context", timeout=30.0)
        raise AssertionError("rank 0 went on without rank 1")
    except RuntimeError as exc:
        assert "rank 1 of this attempt failed" in str(exc) and "device index out of range" in str(exc)
    assert time.time() - t0 < 5.0
    # and the ordinary case: both arrive, both go on; values travel
    c, d = bench.Rendezvous(str(tmp_path), 1, 0, 2), bench.Rendezvous(str(tmp_path), 1, 1, 2)
    d.put("context_1", b"1")
    c.all_ready("context", timeout=5.0)
    d.put("result_1", json.dumps({"x": 2}).encode())
    assert c.gather_json("result", {"x": 1}, timeout=5.0) == [{"x": 1}, {"x": 2}]


def test_dump_outputs_writes_float_arrays_within_budget_with_a_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs without a device: dump_outputs against a stand-in for the library's read-back calls.  Every file is
    float32 / float64, the whole stays under the budget when the coordinates and lattices would not fit, and the sample
    taken then is the same from run to run."""
    import ctypes as C
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 19) + 30000)
    monkeypatch.setattr(bench, "DUMP_POINT_BYTES", 1 << 19)
    n_images, n_pts, dims = 5, 60000, [(4, 4, 5), (9, 9, 11)]

    class FakeLib:
        def frog_get_points(self, ctx, xyz, xyz2):
            a = np.ctypeslib.as_array(xyz2, (n_pts, 3))
            a[:] = np.arange(3 * n_pts, dtype=np.float32).reshape(n_pts, 3)
            return 0

        def frog_get_linear(self, ctx, i, m):
            np.ctypeslib.as_array(m, (16,))[:] = np.eye(4).ravel() * (i + 1)
            return 0

        def frog_get_em(self, ctx, i, v):
            np.ctypeslib.as_array(v, (3,))[:] = (i, 2 * i, 0.5)
            return 0

        def frog_num_grids(self, ctx):
            return len(dims)

        def frog_get_grid(self, ctx, image, k, info, coeffs, cap):
            info._obj.dims[:] = dims[k]
            if coeffs:
                g = int(np.prod(dims[k]))
                assert cap == 3 * g and 0 <= image < n_images
                np.ctypeslib.as_array(coeffs, (3 * g,))[:] = 1000 * k + image
            return 0

    class FakePairs:
        point_offset = np.linspace(0, n_pts, n_images + 1).astype(np.uint64)
    FakePairs.n_images = n_images
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), FakeLib(), C.c_void_p(), FakePairs(), 12.5)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert files == ["em_mixtures.npy", "final_E.npy", "lattice000_coeffs.npy", "lattice001_coeffs.npy", "linear_matrices.npy",
                     "points_xyz2.npy"]
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
        total += a.nbytes
    assert total <= bench.DUMP_BYTES
    xyz2 = np.load(tmp_path / "a" / "points_xyz2.npy")
    assert xyz2.nbytes <= bench.DUMP_POINT_BYTES and len(xyz2) < n_pts
    assert np.all(np.diff(xyz2[:, 0]) > 0) and np.all(xyz2[:, 0] % 3 == 0)     # rows of the whole table, in order
    lat = np.load(tmp_path / "a" / "lattice001_coeffs.npy")
    assert lat.shape[1:] == (9 * 9 * 11, 3) and 1 <= lat.shape[0] < n_images
    assert np.load(tmp_path / "a" / "final_E.npy").tolist() == [12.5]
    assert np.array_equal(np.load(tmp_path / "a" / "linear_matrices.npy")[2], 3 * np.eye(4))
