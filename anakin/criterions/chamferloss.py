from artiboost_amd.criterions import ChamferLoss  # noqa: F401  (anakin/criterions/chamferloss.py:12)
