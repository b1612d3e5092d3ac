#!/usr/bin/env python
"""The edges of a PPO update on the GPU timeline: everything between the step launches.
usage: update_edges.py <dir with *kernel_trace.csv and *memory_copy_trace.csv of ONE rocprofv3 run> [update index, default last]

The run:  rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d <dir> -- python bench.py --gpus 1 --steps 3 --warmup 1
(no counters in the same run).  An update starts at the gather launch of fsrl_ppo_begin and ends with the last step launch before the
next update's gather.  Prints every event of the chosen update that is not a minibatch step launch (ppo_fwd_bwd_kernel /
ppo_wgrad_kernel), with its duration and the idle gap in front of it, then the sums: step launches, the gaps between them, and the rest."""
import csv
import glob
import statistics
import sys

STEP = ("ppo_fwd_bwd_kernel", "ppo_wgrad_kernel")


def load(d):
    ev = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "")))
    for f in glob.glob(d + "/**/*memory_copy_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Direction"].replace("MEMORY_COPY_", "copy ")))
    ev.sort()
    return ev


def main():
    ev = load(sys.argv[1])
    starts = [i for i, e in enumerate(ev) if e[2].startswith("batch_gather")]
    which = int(sys.argv[2]) if len(sys.argv) > 2 else len(starts) - 1
    i0 = starts[which]
    i1 = starts[which + 1] if which + 1 < len(starts) else len(ev)
    # an update ends at its last step launch; what follows (state_restore's copies, the next begin's uploads) is listed after it
    last_step = max(i for i in range(i0, i1) if ev[i][2].startswith(STEP))
    # lead-in: events after the previous update's last step launch
    lead = i0
    while lead > 0 and not ev[lead - 1][2].startswith(STEP):
        lead -= 1
    print(f"update {which}: {last_step - i0 + 1} events from the gather to the last step launch, {i0 - lead} in front of the gather")
    print(f"{'t [us]':>10s} {'gap [us]':>9s} {'dur [us]':>9s}  event")
    t0 = ev[i0][0]
    step_dur, step_gap, rest_dur, rest_gap, n_step = 0.0, 0.0, 0.0, 0.0, 0
    prev_end = ev[lead - 1][1] if lead > 0 else ev[lead][0]
    gaps_between_steps = []
    for i in range(lead, min(last_step + 12, len(ev))):
        s, e, n = ev[i]
        gap, dur = (s - prev_end) / 1e3, (e - s) / 1e3
        is_step = n.startswith(STEP)
        inside = i0 <= i <= last_step
        if is_step and inside:
            step_dur += dur; n_step += 1
            if ev[i - 1][2].startswith(STEP):
                step_gap += max(gap, 0.0); gaps_between_steps.append(gap)
            else:
                rest_gap += max(gap, 0.0)
                print(f"{(s - t0) / 1e3:10.1f} {gap:9.2f} {dur:9.2f}  {n}   <- first step launch after the above")
        else:
            if inside:
                rest_dur += dur; rest_gap += max(gap, 0.0)
            tag = "" if inside else "   (outside the update)"
            print(f"{(s - t0) / 1e3:10.1f} {gap:9.2f} {dur:9.2f}  {n}{tag}")
        prev_end = max(prev_end, e)
    wall = (ev[last_step][1] - ev[i0][0]) / 1e3
    print(f"gather -> last step launch: {wall:.1f} us;  {n_step} step launches {step_dur:.1f} us, gaps between consecutive step launches "
          f"{step_gap:.1f} us (median {statistics.median(gaps_between_steps):.2f});  other events {rest_dur:.1f} us, gaps around them {rest_gap:.1f} us")


if __name__ == "__main__":
    main()
