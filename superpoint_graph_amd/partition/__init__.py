"""Device-side pieces of the reference's `partition/` preprocessing that feed the learning hot path (SURVEY.md section 8, row
f4 tail): `graphs.compute_graph_nn` / `compute_graph_nn_2` (kNN graphs), `graphs.compute_sp_graph` after the triangulation,
ply_c's `compute_geof` and `prune`, and `provider.interpolate_labels` (1-NN label upsampling)."""
