"""A/B of two builds of the library on the world-per-wavefront kernel with the
exact LCP: 512 iCub-class humanoids and 2048 quadrupeds standing under the
PID hold from perturbed postures, 100 warm-up steps, then the best of three
timed runs of 300 device-resident steps; prints us per step, the unconverged
world-steps and a hash of the final state records (equal hashes: the two
builds computed the same bits).  One library per process:
    MWSTEP_LIB=/path/to/libmwstep.so python scripts/ab_wave_lib.py"""
import hashlib
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gym-ignition_amd", "python"))
import numpy as np  # noqa: E402

from mwstep import get_model_file  # noqa: E402
from mwstep import native as N  # noqa: E402
from mwstep.models import ICUB_POSE, icub_posture  # noqa: E402
from mwstep.sim import Simulator  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(os.path.dirname(N.LIB_PATH))
for model, W in (("icub", 512), ("quadruped", 2048)):
    pose0 = {"icub": ICUB_POSE, "quadruped": (0, 0, 0.45, 1, 0, 0, 0)}[model]
    sim = Simulator(get_model_file(model), n_worlds=W, pgs_iters=50, pose=pose0)
    names = sim.joint_names
    sim.set_ground_plane(True, 1.0)
    sim.enable_contacts(True)
    sim.set_controller_period(1e-3)
    for d, n in enumerate(names):
        stiff = any(k in n for k in ("hip", "knee", "ankle", "torso")) or model == "quadruped"
        p, dd = (500.0, 5.0) if stiff else (50.0, 0.5)
        sim.set_pid(d, [p, 0.0, dd, -80.0, 80.0, 0.0, 0.0, -1.0])
    sim.set_control_mode(N.MODE_POSITION)
    rng = np.random.default_rng(1)
    home = np.array([0.6, -1.2] * 4 if model == "quadruped" else icub_posture(names))
    sim.set("reset_q", home + rng.uniform(-0.05, 0.05, (W, len(names))))
    sim.set("position_target", np.tile(home, (W, 1)))
    sim.run(paused=True)
    sim.run_device(100)
    sim.get("q")
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        sim.run_device(300)
        sim.get("q")
        best = min(best, (time.perf_counter() - t0) / 300)
    digest = hashlib.sha256(sim.get_state().tobytes()).hexdigest()[:12]
    print(f"{label:>10} {model} W={W}: {best * 1e6:8.1f} us/step, unconverged {sim.lcp_unconverged()}, state {digest}",
          flush=True)
    sim.close()
