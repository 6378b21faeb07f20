"""Device op dispatch.

Policy: on a GPU tensor the hand-written HIP kernels (greptimedb_amd._hip_ops,
gfx950) are the ONLY path — if the extension is missing we raise
NativeExtensionMissing rather than silently falling back to eager PyTorch.
CPU tensors use the reference implementations in ops.cpu_ref (plain
PyTorch/f64), which double as the numerics oracle for GPU tests.
"""

from greptimedb_amd.ops.kernels import (  # noqa: F401
    bucket_cells,
    dedup_mark_last,
    filter_series_time,
    gorilla_encode,
    grouped_moments,
    grouped_quantile,
    hip_ops_available,
    merge_last_non_null,
    moments_finish,
    prom_range_eval,
    quantile_lerp,
    series_last,
    ts_bucket_agg,
    ts_bucket_agg_acc,
    ts_bucket_agg_finish,
)
