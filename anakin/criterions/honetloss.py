from artiboost_amd.criterions import ManoLoss, ObjLoss  # noqa: F401  (anakin/criterions/honetloss.py:12,77)
