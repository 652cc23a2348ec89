"""Largest err / bound per (entry, output, act) and state of the GEMM form tests, from the figures tests/test_gpu_gemm_forms.py prints:

    python -m pytest tests/test_gpu_gemm_forms.py -m gpu -s | python tools/gemm_forms_summary.py > profiles/gemm_forms.txt

One line per (entry, output, act): per state (edge shapes at a K-step state, a walk shape, a split shape, a K share of the skinny kernel)
the max over all of its cases of max(err / bound) -- the elementwise bound of tests/gemm_forms.py, 1 = at the bound."""
import collections
import sys


def main():
    rows = collections.OrderedDict()
    for line in sys.stdin:
        line = line.lstrip(".FE").rstrip()                      # pytest's progress marks precede a test's first line
        if not line.startswith("gemm_forms |"):
            continue
        _, entry, out, act, state, ratio = [f.strip() for f in line.split("|")]
        states = rows.setdefault((entry, out, act), collections.OrderedDict())
        states[state] = max(states.get(state, 0.0), float(ratio))
    for (entry, out, act), states in rows.items():
        print("%-22s %-10s %-9s %s" % (entry, out, act, "   ".join("%s: %.3f" % kv for kv in states.items())))


if __name__ == "__main__":
    main()
