"""One process under one setting of the library's read-once switches (``tests/test_gpu_variants.py`` starts it with
the switches in its environment): a small context, every comparison of ``tests/_variant_cases.py``, then one JSON
line ``{"ran": n, "failures": [...], "stopped": why or null}``.  The exit status is 0 only if every comparison ran
and none failed.  The first error that is not a difference of bytes ends the run: nothing more is started on a GPU
that has just refused a launch or faulted."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "distributed-video-filter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> int:
    import numpy as np

    import _variant_cases as V
    import vfilter

    ran, failures, stopped = 0, [], None
    with vfilter.Context(0, max_frame_bytes=2 << 20, max_batch=1) as ctx:
        for name, run in V.comparisons():
            try:
                got, want = run(ctx)
            except Exception as e:  # a refused launch, a HIP error, a canary: stop here
                stopped = "%s: %s: %s" % (name, type(e).__name__, e)
                break
            ran += 1
            got, want = np.asarray(got), np.asarray(want)
            if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(got, want):
                where = np.argwhere(got.reshape(-1) != want.reshape(-1))[:3].reshape(-1).tolist() if got.size == want.size else []
                failures.append("%s: differs at %s" % (name, where))
    print(json.dumps({"ran": ran, "failures": failures, "stopped": stopped}), flush=True)
    return 0 if not failures and stopped is None and ran == V.EXPECTED else 1


if __name__ == "__main__":
    sys.exit(main())
