from artiboost_amd.metrics import InteractionMetric, ObjectMeshTable  # noqa: F401  (no counterpart in the reference: DESIGN.md section 24)
