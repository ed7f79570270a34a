from artiboost_amd.fitting import IKNet, IKNetHIP  # noqa: F401  (anakin/postprocess/iknet/model.py:6)
