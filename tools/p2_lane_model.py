#!/usr/bin/env python3
"""Event model of the two-lane look-ahead protocol of the persistent SGHMC kernel (csrc/hmcx_persist2.hip,
DESIGN §5.1 rounds 9 and 10).  Host arithmetic only; every figure it prints is a model, not a measurement.

Lane s & 1 runs step s.  A run of step s costs `step + leap * n(s)` µs in a lane, n(s) leapfrogs, uniform on
0 … nmax; of `step`, `tail` µs (the accept round) lie behind the last leapfrog and the rest before the first.
A step moves the state with probability `rate` when n(s) > 0.  Step s is final once V(s − 1) is known: the
verdict read plus the publish of V(s) cost `verdict` µs; when step s − 1 moved the state, the run is void and
the step is run again from the true state (state gather `verdict`, the run, the publish `verdict`).

Variants (`variant=`):
  parent     a voided run is finished before it is redone (round 9);
  stop       a voided run is left at the first leapfrog boundary at or after the arrival of V(s − 1) =
             changed, plus `late` boundaries (0: the next boundary, 1: one iteration later); a verdict that
             lands in the last `late + 1` iterations changes nothing;
  run_on     a lane whose verdict is pending at the end of its run starts its next step at once and
             resolves the verdict only at the end of that next run.
  run_on_poll  (`lanes_run_on_poll`, round 11) `stop` with `late`, and a lane whose run of step s ends with
             V(s − 1) unknown and with the own decision "state unchanged" parks the step and starts step s + 2
             at once; the poll of that run resolves V(s − 1): unchanged is seen `seen` µs after the next
             boundary and V(s) published `seen` µs later; changed voids step s and the run, which the lane
             leaves `late` boundaries on, gathers the state, redoes s and then runs s + 2 again.  One step
             per lane may be parked (`pending=1`): a run that ends with the parked step unresolved waits for
             its verdict before the accept round.
`overhead` µs are added to every leapfrog in a lane (the price of a poll inside the iteration).

    python tools/p2_lane_model.py [--rate 0.092] [--steps 200000]
"""
import argparse
import random

R9 = dict(step=10.4, leap=7.6, verdict=1.5, tail=3.0, rate=0.092, nmax=19)   # round-9 coefficients
SERIAL = dict(step=7.42, leap=7.29)                                          # the helper launch's fit


def schedule(steps, rate, nmax, seed=1):
    rng = random.Random(seed)
    n = [rng.randint(0, nmax) for _ in range(steps)]
    moved = [k > 0 and rng.random() < rate for k in n]
    return n, moved


def lanes(n, moved, variant="parent", late=0, overhead=0.0, step=10.4, leap=7.6, verdict=1.5, tail=3.0, **_):
    """µs per chain step and the share of lane time spent waiting for a verdict."""
    lf = leap + overhead
    head = step - tail
    S = len(n)
    dur = [step + lf * k for k in n]
    fin = [0.0] * S
    free = [0.0, 0.0]
    wait = 0.0
    ran_on = [False] * S              # run_on: the run of step s ended before the lane's previous step was final
    for s in range(S):
        ln = s & 1
        start = free[ln]
        end = start if ran_on[s] else start + dur[s]
        if s == 0:
            fin[s] = end + verdict
            free[ln] = fin[s]
            continue
        vt = fin[s - 1]
        if variant == "run_on" and vt > end and s + 2 < S and not ran_on[s]:
            e2 = end + dur[s + 2]
            t = max(e2, vt)
            wait += t - e2
            if not moved[s - 1]:
                fin[s] = t + verdict
                ran_on[s + 2] = not moved[s]
            else:
                fin[s] = t + 2 * verdict + dur[s]
            free[ln] = fin[s]
            continue
        t = max(end, vt)
        if moved[s - 1] and variant == "stop" and vt < end and not ran_on[s]:
            # boundary i of the run (i iterations done) lies head + lf·i behind its start; the run can be
            # left at the boundaries 0 … n − 1
            i = 0
            while start + head + lf * i < vt:
                i += 1
            if i + late <= n[s] - 1:
                t = start + head + lf * (i + late)
        wait += max(0.0, vt - end)
        fin[s] = t + verdict if not moved[s - 1] else t + 2 * verdict + dur[s]
        free[ln] = fin[s]
    total = max(fin[-1], fin[-2] if S > 1 else 0.0)
    return total / S, wait / (2.0 * total)


def lanes_run_on_poll(n, moved, pending=1, late=1, seen=1.0, overhead=0.0, step=10.4, leap=7.6, verdict=1.5, tail=3.0,
                      **_):
    """µs per chain step, the share of steps parked and the share of steps parked and then voided."""
    if pending != 1:
        raise ValueError("one parked step per lane is all the kernel's slots allow")
    lf = leap + overhead
    head = step - tail
    S = len(n)
    dur = [step + lf * k for k in n]
    fin = [0.0] * S
    free = [0.0, 0.0]
    hold = [0.0] * (S + 2)            # the accept round of the run of step s starts no earlier (a parked s − 2)
    parked = voided = 0

    def boundary(start, k, t):
        """First boundary i of a run of k leapfrogs started at `start` that lies at or after t, or None."""
        i = 0
        while i < k and start + head + lf * i < t:
            i += 1
        return i if i < k else None

    for s in range(S):
        ln = s & 1
        start = free[ln]
        end = max(start + dur[s] - tail, hold[s]) + tail
        if s == 0:
            fin[s] = end + verdict
            free[ln] = fin[s]
            continue
        vt = fin[s - 1]
        can_park = vt > end and not moved[s] and s + 2 < S and n[s + 2] > 0
        if can_park:
            parked += 1
            s2 = end                                  # the run of s + 2 starts here
            i = boundary(s2, n[s + 2], vt)
            if not moved[s - 1]:
                free[ln] = s2
                if i is not None:
                    fin[s] = s2 + head + lf * i + 2 * seen
                else:                                 # resolved in the blocking wait before the accept round
                    fin[s] = max(s2 + dur[s + 2] - tail, vt) + verdict
                    hold[s + 2] = fin[s]
            else:
                voided += 1
                if i is not None and i + late <= n[s + 2] - 1:
                    t = s2 + head + lf * (i + late)
                else:
                    t = max(s2 + dur[s + 2] - tail, vt)
                fin[s] = t + 2 * verdict + dur[s]
                free[ln] = fin[s]
            continue
        t = max(end, vt)
        if moved[s - 1] and vt < end:
            i = boundary(start, n[s], vt)
            if i is not None and i + late <= n[s] - 1:
                t = start + head + lf * (i + late)
        fin[s] = t + verdict if not moved[s - 1] else t + 2 * verdict + dur[s]
        free[ln] = fin[s]
    total = max(fin[-1], fin[-2] if S > 1 else 0.0)
    return total / S, parked / float(S), voided / float(S)


def serial(n, step=7.42, leap=7.29):
    return (step * len(n) + leap * sum(n)) / len(n)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200000)
    ap.add_argument("--seed", type=int, default=1)
    for k, v in R9.items():
        ap.add_argument("--" + k, type=type(v), default=v)
    a = ap.parse_args()
    co = {k: getattr(a, k) for k in R9}
    n, moved = schedule(a.steps, a.rate, a.nmax, a.seed)
    ser = serial(n, **SERIAL)
    base, w = lanes(n, moved, **co)
    print("serial %.1f us per step; accept rate %.3f" % (ser, a.rate))
    print("parent                       %.1f us per step (x%.3f), verdict wait %.1f %%" % (base, ser / base, 100 * w))
    for name, kw in (("run on, resolve at run end ", dict(variant="run_on")),
                     ("stop at the next boundary  ", dict(variant="stop", late=0)),
                     ("stop one boundary late     ", dict(variant="stop", late=1)),
                     ("  ... leapfrog 0.1 us dearer", dict(variant="stop", late=1, overhead=0.1))):
        v, w = lanes(n, moved, **dict(co, **kw))
        print("%s  %.1f us per step (%+.1f %%), verdict wait %.1f %%" % (name, v, 100 * (v / base - 1), 100 * w))
    stop1, _ = lanes(n, moved, **dict(co, variant="stop", late=1))
    v, pk, vd = lanes_run_on_poll(n, moved, pending=1, late=1, **co)
    print("run on, resolved by the poll  %.1f us per step (%+.1f %% on stop one boundary late), parked %.2f, voided %.3f "
          "of the steps" % (v, 100 * (v / stop1 - 1), pk, vd))


if __name__ == "__main__":
    main()
