"""The launches of the update paths, for a comparison of two builds (refactoring check; MOBROB_PPO_LIB selects the library):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scratch/update_launches.py run
    python3 scratch/update_launches.py summary DIR_A DIR_B
  or, without a profiler, from the HIP runtime's own log (every API call with its arguments, every dispatch with its kernel name):
    AMD_LOG_LEVEL=3 python3 scratch/update_launches.py run 2> LOG
    python3 scratch/update_launches.py hiplog LOG_A LOG_B
`run`: one collect_synthetic + train() in each of seven modes -- 2x256 chain kernel, 2x64 epoch kernel, 2x64 three launches per
step (split kernel), 2x64 block kernel, 2x64 pair kernel with the narrow and with the wide reduce, generic chain (2x48).
`summary` / `hiplog`: the sequence of (kernel, grid, workgroup) of the two traces in start order -- `hiplog`: of launches, copies,
memsets, event records and waits with their sizes, and of dispatched kernel names -- compared line for line, and printed with
repeated blocks folded."""
import gzip, itertools, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    from mobrob_amd.engine import PPOEngine
    modes = [("2x256 chain", dict(D=58, A=12, H=256, N=128, T=32, B=1024), None),
             ("2x64 epoch kernel", dict(D=58, A=12, H=64, N=16, T=125, B=100), 1),
             ("2x64 three launches", dict(D=58, A=12, H=64, N=16, T=125, B=100), 0),
             ("2x64 block", dict(D=14, A=2, H=64, N=256, T=64, B=2048), 0),   # under MOBROB_SPLIT64_MAX_TILES=0
             ("2x64 pair", dict(D=14, A=2, H=64, N=512, T=32, B=4096), 0),
             ("2x64 pair, wide reduce", dict(D=14, A=2, H=64, N=1024, T=32, B=16384), 0),
             ("generic chain", dict(D=26, A=2, H=48, N=64, T=32, B=256), 0)]
    for name, s, mode in modes:
        if name == "2x64 block":
            os.environ["MOBROB_SPLIT64_MAX_TILES"] = "0"
        e = PPOEngine(obs_dim=s["D"], act_dim=s["A"], n_envs=s["N"], n_steps=s["T"], batch_size=s["B"], n_epochs=2,
                      pi=(s["H"], s["H"]), vf=(s["H"], s["H"]), ent_coef=0.01, seed=5)
        os.environ.pop("MOBROB_SPLIT64_MAX_TILES", None)
        if name == "2x64 three launches":
            e.set_hyper(epoch_kernel=0)
        e.collect_synthetic(p_term=0.02, time_limit=40)
        e.train(None)
        assert mode is None or e.update_mode() == mode, (name, e.update_mode())
        e.close()


def sequence(d):
    from rollout_launches import launches
    _, queues = launches(d)
    return [[k[:3] for k in q] for q in queues]


def hip_log(path):
    """One entry per enqueueing HIP call (name + arguments, addresses masked) and per dispatched kernel of an AMD_LOG_LEVEL=3 log."""
    import re
    calls = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel", "hipLaunchCooperativeKernel",
             "hipMemcpyAsync", "hipMemcpy2DAsync", "hipMemsetAsync", "hipMemcpy", "hipEventRecord", "hipStreamWaitEvent")
    seq = []
    for ln in (gzip.open(path, "rt", errors="replace") if path.endswith(".gz") else open(path, errors="replace")):
        m = re.search(r"ShaderName : (.*?)\s*(\x1b\[0m)?$", ln.rstrip())
        if m:
            seq.append(("kernel " + m.group(1), "", ""))
            continue
        m = re.search(r"\b(hip\w+) \( (.*) \)\s*(\x1b\[0m)?$", ln.rstrip())
        if m and m.group(1) in calls:
            seq.append((m.group(1), re.sub(r"0x[0-9a-f]+|stream:<[^>]*>|char array:<[^>]*>", "*", m.group(2)), ""))
    return [seq]


def summary(da, db, read=sequence):
    qa, qb = read(da), read(db)
    print(f"queues: {len(qa)} / {len(qb)}, launches per queue: {[len(q) for q in qa]} / {[len(q) for q in qb]}")
    print("sequence of (kernel, grid, workgroup), line for line:", "EQUAL" if qa == qb else "DIFFERENT")
    for a, b in zip(qa, qb):
        for i, (x, y) in enumerate(itertools.zip_longest(a, b)):
            if x != y:
                print(f"    first difference at launch {i}: {x} | {y}")
                break
    for q in qa:   # repeated blocks of up to 24 launches (the steps of an epoch) are printed once with their count
        i = 0
        while i < len(q):
            p, reps = 1, 1
            for cand in range(1, 25):
                r = 1
                while q[i + r * cand:i + (r + 1) * cand] == q[i:i + cand]:
                    r += 1
                if r > 1 and cand * r > p * reps:
                    p, reps = cand, r
            print(f"  {reps} x" + (" {" if p > 1 else ""))
            for k in q[i:i + p]:
                print(f"        {k[0][:100]:<100} grid {k[1]} wg {k[2]}")
            if p > 1:
                print("  }")
            i += p * reps


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else summary(sys.argv[2], sys.argv[3], hip_log if sys.argv[1] == "hiplog" else sequence)
