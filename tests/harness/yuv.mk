# tests/harness/yuv.mk — ASan + UBSan build of yuv_check (tests/test_yuv_core.py): the 4:2:2 / 4:4:4
# device-picture core (csrc/jmh_yuv.h) against the formulas of include/jmhip_yuv.h and jm_pad_picture
# of host/yuv.c.  Everything is compiled from source with the sanitizers:   make -C tests/harness -f yuv.mk
CC       ?= gcc
ASAN     := _build_asan
HOSTDIR  := ../../h264-jm-commentary_amd/host
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS     := $(HOSTDIR)/jmhost.h $(CSRC)/jmh_yuv.h $(CSRC)/jmh_ingest.h

$(ASAN)/yuv_check: yuv_check.c $(HOSTDIR)/yuv.c $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) -I$(HOSTDIR) -I../../include yuv_check.c $(HOSTDIR)/yuv.c -o $@
