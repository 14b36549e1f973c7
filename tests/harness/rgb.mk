# tests/harness/rgb.mk — ASan + UBSan build of rgb_check (tests/test_rgb_core.py): the RGB
# device-picture core (csrc/jmh_rgb.h) against its formulas and jm_pad_picture of host/yuv.c.
# Everything is compiled from source with the sanitizers:   make -C tests/harness -f rgb.mk
CC       ?= gcc
ASAN     := _build_asan
HOSTDIR  := ../../h264-jm-commentary_amd/host
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS     := $(HOSTDIR)/jmhost.h $(CSRC)/jmh_rgb.h $(CSRC)/jmh_ingest.h

$(ASAN)/rgb_check: rgb_check.c $(HOSTDIR)/yuv.c $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) -I$(HOSTDIR) -I../../include rgb_check.c $(HOSTDIR)/yuv.c -lm -o $@
