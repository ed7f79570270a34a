from artiboost_amd.metrics import MeanAlignedEPE, MeanSurfaceDist, MeshFScore  # noqa: F401  (no counterpart in the reference: DESIGN.md section 23)
