from artiboost_amd.criterions import AlignLoss  # noqa: F401  (anakin/criterions/alignloss.py:13)
