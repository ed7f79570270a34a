from artiboost_amd.draw import MeshDrawer, draw_skeleton  # noqa: F401  (anakin/viztools/draw.py: save_a_image_with_mesh_joints_objects, draw_2d_skeleton)
