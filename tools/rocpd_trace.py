#!/usr/bin/env python
"""List the individual dispatches of kernels matching a substring from a rocprofv3 rocpd database, in start order.

    python tools/rocpd_trace.py x_results.db icp_pass [max_rows]
    python tools/rocpd_trace.py x_results.db --launches      # every dispatch without its times: diff two runs' output
"""
import sqlite3
import sys


def main(path, needle, limit=200):
    c = sqlite3.connect(path)
    views = [r[0] for r in c.execute("select name from sqlite_master where type in ('view','table')")]
    src = "kernels" if "kernels" in views else None
    if src is None:
        print("views/tables:", views)
        return
    cols = [r[1] for r in c.execute(f"pragma table_info({src})")]
    print("#", cols)
    q = f"select name, start, end, (end-start)/1000.0 from {src} where name like ? order by start limit ?"
    t0 = None
    for name, st, en, us in c.execute(q, (f"%{needle}%", limit)):
        t0 = t0 or st
        print(f"{(st - t0) / 1000.0:12.1f} us  +{us:9.1f} us  {name.split('(')[0][:70]}")


def launches(path):
    """Every dispatch as kernel name, grid and workgroup size, queue by queue in start order, the queues numbered by first use: two runs that sent
    the same commands to the device print the same text."""
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    queue = [x for x in cols if "queue" in x.lower()]
    shape = [x for x in cols if "grid" in x.lower() or "workgroup" in x.lower()]
    if not queue or not shape:
        raise SystemExit(f"no queue / grid / workgroup columns among {cols}")
    print("#", queue[0], shape)
    rows = c.execute(f"select {queue[0]}, name, {', '.join(shape)} from kernels order by start").fetchall()
    first_use = {}
    for r in rows:
        first_use.setdefault(r[0], len(first_use))
    for qid, k in sorted(first_use.items(), key=lambda kv: kv[1]):
        mine = [r for r in rows if r[0] == qid]
        print(f"== queue {k}: {len(mine)} launches")
        for r in mine:
            print(r[1].split("(")[0], *r[2:])


if __name__ == "__main__":
    if sys.argv[2] == "--launches":
        launches(sys.argv[1])
        sys.exit(0)
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 200)
