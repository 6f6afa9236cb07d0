"""rocprofv3 --kernel-trace --stats CSV -> markdown summary under profiles/.
usage: python scripts/summarize_profile.py <kernel_stats.csv> <out.md> <steps in trace> "<title>" [bench line .json of the traced run]
The sentence about what the sum of kernel durations means follows the stepper state of the bench line ("stepper": wgrad_side_stream, and
coarse_window where the line carries it); without a bench line it describes the fp32 default of pulpo_amd.dp."""
import csv, json, os, sys
src, out, nsteps, title = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]


def schedule_note():
    st = {}
    if len(sys.argv) > 5:
        st = json.loads(open(sys.argv[5]).read().strip().splitlines()[-1]).get("stepper") or {}
    if st.get("wgrad_side_stream"):
        return ("weight-gradient kernels run on a second stream concurrently with the main stream, so this sum exceeds the wall time per step and "
                "overlapped kernels show stretched durations")
    window = st.get("coarse_window")
    if window is None:                             # (bench lines do not carry it: the default of the stepper)
        dp = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pulpo_amd", "dp.py")).read()
        window = "\nCOARSE_WINDOW = True" in dp
    if window:
        return ("weight-gradient kernels run in line on the main stream, except those of the coarse pyramid levels and the few held back for them, "
                "which run on a second stream beside the coarse levels' kernels on a capped grid: there the sum exceeds the wall time and "
                "overlapped kernels show stretched durations")
    return "every kernel runs in line on one stream: the sum is the GPU-busy time of the step"


rows = list(csv.DictReader(open(src)))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
with open(out, "w") as f:
    f.write(f"# {title}\n\n160^3 fp32, T5/L4, B=1, one MI355X; {nsteps} steps in the trace.  Source CSV next to this file.\n")
    f.write(f"\nSum of kernel durations {tot/1e6:.1f} ms = {tot/1e6/nsteps:.2f} ms/step ({schedule_note()})\n\n"
            f"| kernel | calls/step | ms/step | avg us | % |\n|---|---|---|---|---|\n")
    for r in rows[:45]:
        n = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "")
        n = n.split("(")[0] if not n.startswith("at::") else n[:70]
        f.write(f"| `{n}` | {int(r['Calls'])/nsteps:.1f} | {float(r['TotalDurationNs'])/1e6/nsteps:.3f} | {float(r['AverageNs'])/1e3:.1f} | {float(r['Percentage']):.1f} |\n")
print(open(out).read()[:1800])
