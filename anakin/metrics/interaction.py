from artiboost_amd.metrics import IA_SYM_MEASURES, InteractionMetric, ObjectMeshTable, interaction_sym_values_torch  # noqa: F401  (no counterpart in the reference: DESIGN.md sections 24, 27)
