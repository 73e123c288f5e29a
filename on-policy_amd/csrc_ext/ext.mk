# Entry points added to libmappo_hip.so after the round-6 kernel sources were frozen: csrc/ stays byte-identical, because
# bench.py's csrc_digest() and profiles/kernel_resources.json tie the committed profiles to exactly those sources.
# Read after csrc/Makefile, from csrc/:
#     make -C on-policy_amd/csrc -f Makefile -f ../csrc_ext/ext.mk ARCH=gfx950
# The sources join SRCS, so the library's link line (which expands OBJS when it runs), `clean` and `resource-usage`
# take them as well.
EXT_SRCS = ../csrc_ext/mappo_env_reference.hip ../csrc_ext/mappo_sample_multi.hip
SRCS    += $(EXT_SRCS)

$(OUT): $(EXT_SRCS:.hip=.o)
