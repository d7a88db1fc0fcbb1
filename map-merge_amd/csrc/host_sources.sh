# The translation units of libmm3d.so that hold no kernel, in one list: map-merge_amd/build.sh builds them into the library,
# and tests/host_san/build.sh and tests/host_san_cache/build.sh compile the same files, unchanged, against their fake device.
# (map_cache.cpp is not in it: tests/host_san links without the map cache, and the two others name it themselves.)
MM3D_HOST_SOURCES="runtime.cpp linalg.cpp host_pipeline.cpp devices.cpp capi.cpp stage_rules.cpp pair_estimate.cpp driver_streams.cpp driver_shard.cpp driver_devices.cpp"
