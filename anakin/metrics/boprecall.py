from artiboost_amd.metrics import BOPRecall  # noqa: F401  (no counterpart in the reference, whose VSD / MSPD are stubs: DESIGN.md section 25)
