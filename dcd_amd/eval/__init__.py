"""KITTI average precision on the device: annotation files, ignore rules, overlap and matching kernels, AP tables."""
