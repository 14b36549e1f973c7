# tests/harness/ingest.mk — ASan + UBSan build of ingest_check (tests/test_ingest_core.py): the
# device-picture core (csrc/jmh_ingest.h) against jm_pad_picture of host/yuv.c.  Everything is
# compiled from source with the sanitizers:   make -C tests/harness -f ingest.mk
CC       ?= gcc
ASAN     := _build_asan
HOSTDIR  := ../../h264-jm-commentary_amd/host
CSRC     := ../../h264-jm-commentary_amd/csrc
SANFLAGS := -O2 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
HDRS     := $(HOSTDIR)/jmhost.h $(CSRC)/jmh_ingest.h

$(ASAN)/ingest_check: ingest_check.c $(HOSTDIR)/yuv.c $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu11 -Wall -Wno-unused-function $(SANFLAGS) -I$(HOSTDIR) -I../../include ingest_check.c $(HOSTDIR)/yuv.c -o $@
