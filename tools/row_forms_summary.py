"""Largest observed error per entry and register form of the row passes, from the figures tests/test_gpu_row_forms.py prints:

    python -m pytest tests/test_gpu_row_forms.py -m gpu -s | python tools/row_forms_summary.py > profiles/row_forms.txt

One line per (entry, form): the widths and row counts that reached it and, per figure, the max over all of them."""
import collections
import re
import sys

LINE = re.compile(r"row_forms (.+?)\s+(form \S+|nch \d)\s+d\s+(\d+)( off4)? n\s+(\d+)\s+(.*)")


def main():
    rows = collections.OrderedDict()
    for line in sys.stdin:
        m = LINE.match(line.lstrip(".").rstrip())               # pytest's progress dots precede a test's first line
        if not m:
            continue
        entry, form, d, off, n, figures = m.groups()
        rec = rows.setdefault((entry.strip(), form + (off or "")), {"d": set(), "n": set(), "figures": collections.OrderedDict()})
        rec["d"].add(int(d))
        rec["n"].add(int(n))
        tokens = figures.split()
        for name, value in zip(tokens[::2], tokens[1::2]):
            name = re.sub(r"_c[13]$", "", name)                 # one figure for both class counts
            rec["figures"][name] = max(rec["figures"].get(name, 0.0), float(value))
    for (entry, form), rec in rows.items():
        print("%-22s %-14s d %-10s n %-20s %s" % (entry, form, ",".join(map(str, sorted(rec["d"]))), ",".join(map(str, sorted(rec["n"]))),
                                                 "  ".join("%s %.2e" % kv for kv in rec["figures"].items())))


if __name__ == "__main__":
    main()
