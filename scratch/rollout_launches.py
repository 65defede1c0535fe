"""The launches of the rollout paths, for a comparison of two builds under rocprofv3 (refactoring check):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scratch/rollout_launches.py run   (MOBROB_PPO_LIB selects the library)
    python3 scratch/rollout_launches.py summary DIR_A DIR_B
`run`: one device rollout and one served host rollout (native C env, two row ranges) at each width, one act / store step.
`summary`: the multiset of (kernel, grid, workgroup, LDS bytes) and the kernel order per stream of the two traces, compared."""
import collections, csv, glob, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    from mobrob_amd.engine import PPOEngine
    from mobrob_amd.envs.native_env import NativeGoalVecEnv
    from mobrob_amd.envs.wrapper import ROBOT_DIMS
    D, A, _ = ROBOT_DIMS["doggo"]
    os.environ["MOBROB_COLLECT_SERVER"] = "2"
    for H, N, T in ((256, 512, 64), (64, 1024, 256)):    # both cut into chunks with a side-stream value pass
        e = PPOEngine(obs_dim=D, act_dim=A, n_envs=N, n_steps=T, batch_size=N, n_epochs=1, pi=(H, H), vf=(H, H), seed=5)
        e.collect_synthetic(p_term=0.02, time_limit=40)
        e.synchronize()
        env = NativeGoalVecEnv.for_robot("doggo", N, time_limit=5, seed=7)
        b = dict(obs=e.pinned((N, D)), clip=e.pinned((N, A)), rew=e.pinned((N,)), done=e.pinned((N,), np.uint8),
                 trunc=e.pinned((N,), np.uint8), term=e.pinned((N, D)))
        env.use_buffers(obs=b["obs"], rewards=b["rew"], dones=b["done"], truncated=b["trunc"], terminal_obs=b["term"])
        env.reset()
        e.rollout_begin()
        e.part_pipeline(2, b["obs"], b["clip"], b["rew"], b["done"], b["trunc"], b["term"]).collect(env.step_range_fn, env.handle)
        e.rollout_begin()
        e.act(b["obs"], None, out_clipped=b["clip"], want_all=False)
        b["trunc"][:] = 0
        b["trunc"][0] = b["done"][0] = 1
        e.store(b["rew"], b["done"], b["trunc"], b["term"])                                     # pinned buffers
        e.act(np.array(b["obs"]), None)
        e.store(np.array(b["rew"]), np.array(b["done"]), np.array(b["trunc"]), np.array(b["term"]))   # ordinary buffers
        e.synchronize()
        env.close()
        e.close()


def launches(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(f) == 1, f
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    key = lambda r: (r["Kernel_Name"], (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])),
                     (int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"])), int(r["LDS_Block_Size"]))
    per_queue = collections.OrderedDict()
    for r in rows:
        per_queue.setdefault(r["Queue_Id"], []).append(key(r))
    return collections.Counter(key(r) for r in rows), list(per_queue.values())


def summary(da, db):
    (ma, qa), (mb, qb) = launches(da), launches(db)
    print(f"launches: {sum(ma.values())} / {sum(mb.values())}, distinct (kernel, grid, workgroup, LDS): {len(ma)} / {len(mb)}")
    print("multiset of (kernel, grid, workgroup, LDS bytes):", "EQUAL" if ma == mb else "DIFFERENT")
    for k in sorted(set(ma) | set(mb)):
        if ma[k] != mb[k]:
            print("   ", ma[k], mb[k], k)
    # queues in order of first use; the streams of an engine are created in the same order under either library
    print("kernel order per queue (in order of first use):", "EQUAL" if qa == qb else "DIFFERENT", [len(q) for q in qa], [len(q) for q in qb])
    for k, n in sorted(ma.items(), key=lambda kv: kv[0][0]):
        print(f"  {n:5d} x {k[0][:90]:<90} grid {k[1]} wg {k[2]} lds {k[3]}")


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else summary(sys.argv[2], sys.argv[3])
