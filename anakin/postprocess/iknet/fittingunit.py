from artiboost_amd.fitting import FittingUnit  # noqa: F401  (anakin/postprocess/iknet/fittingunit.py:112)
