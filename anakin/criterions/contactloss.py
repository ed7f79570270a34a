from artiboost_amd.criterions import ContactLoss  # noqa: F401  (the contact loss of Hasson et al., CVPR 2019; fingertip ids of anakin/models/mano.py:26-30)
