"""The workload of the counter runs of the messages kernels (profiles/r16_messages.txt): C4 at 1M rows,
AUDIT, the digest, the members of the 32 groups with the most findings, and one Batch.messages over
them (two calls of the library: the first runs the length and scan steps only). Run it under
  rocprofv3 --pmc <one counter group> -d <dir> -o run --output-format csv -- python scripts/messages_pmc.py
one group a run, with no tracing beside the counters; the rows of messages_*_kernel in
<dir>/run_counter_collection.csv are summed per kernel and counter."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "policy-server_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import kwgpu as K
from helpers import config
env = K.EvaluationEnvironment(config("c4_64"), continue_on_errors=True, always_accept_namespace="kubewarden", device=0)
ids = env.policy_ids()
b = K.SynthBatch(4, 1_000_000, seed=4).batch().to_device(0)
b.validate(env, ids, K.AUDIT)
d = b.digest()
recs = np.ascontiguousarray(d.recs[np.argsort(-d.recs["count"].astype(np.int64), kind="stable")][:32])
m = b.digest_members(recs, words=False)
cols = np.repeat(recs["col"].astype(np.uint32), np.diff(m.off.astype(np.int64)))
t = b.messages(env, ids, m.rows, cols)
print("items", m.rows.size, "bytes", t.text.size, b.debug_messages_stats())
