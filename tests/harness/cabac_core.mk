# tests/harness/cabac_core.mk — ASan + UBSan build of cabac_core_check (tests/test_cabac_core.py): the
# device CABAC writer's shared core (csrc/jmh_cabac_write.h) against host/cabac.c, with the CPU
# oracle behind the host plumbing for encoded results.  Everything is compiled from source with the
# sanitizers:   make -C tests/harness -f cabac_core.mk
CC       ?= gcc
ASAN     := _build_asan
ORACLE   := ../../oracle
HOSTDIR  := ../../h264-jm-commentary_amd/host
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
OSRCP    := $(addprefix $(ORACLE)/,common.c encode.c rdo.c cabac_enc.c cavlc_bits.c frame.c decoder.c hbd.c)
HOSTSRCS := $(addprefix $(HOSTDIR)/,cfg.c yuv.c bitstream.c cabac.c deblock.c encoder.c jm86.c cavlc_ref.c cabac_ref.c)
HDRS     := $(ORACLE)/jm_oracle.h $(ORACLE)/jmo_internal.h $(HOSTDIR)/jmhost.h $(HOSTDIR)/bitstream_int.h ../../include/jmhip.h \
            ../../include/jmhip_cavlc.h ../../include/jmhip_cabac.h $(CSRC)/jmh_cabac_write.h $(CSRC)/jmh_cabac_tables.h $(CSRC)/jmh_cavlc_write.h $(CSRC)/jmh_cavlc_rate.h $(CSRC)/jmh_cabac_rate.h

$(ASAN)/cabac_core_check: cabac_core_check.c $(OSRCP) $(HOSTSRCS) $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu99 -Wall $(SANFLAGS) -I$(ORACLE) -I$(HOSTDIR) cabac_core_check.c $(OSRCP) $(HOSTSRCS) -o $@ -lm -lpthread
